"""GPU tests (-m gpu; a context needs a device, nothing is launched by the checks): how a runProgram job's NAMED arguments are found,
type-checked, size-checked and reported (ph_run.cpp: ph_check_program / ph_run_program / ph_run_programs).

One accepted job per kernel id of ph_program.h (several where the argument list has forms), and from each of them defective jobs
derived mechanically, one defect each: an argument removed, a buffer one byte short, a buffer where a number belongs and the
other way round, a plain buffer where an image belongs, zero globalWorkItems / workItemsPerGroup, a packing out of range or one
the channel kernel refuses, a matrix never written through hostAccess, odd sizes for the even-only formats.  Every job goes
through Context.run_program(check_only=True); the return code and the whole ph_last_error text are compared with
tests/data/program_arg_errors.json, which was recorded from the library as it was BEFORE the by-name layer was rewritten around
one argument reader (`PYTHONPATH=. python tests/test_program_args_gpu.py` records it - from the library PHANERON_HIP_LIB names).  The accepted
jobs of the programs that fold several arguments are also run, against the typed calls, bit for bit."""
import json
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest

import frames
import packfmt
from phaneron_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "data", "program_arg_errors.json")
W, H, WIPG = 192, 8, 16
LUT = 65536 * 4


class B:
    """a buffer argument: its size, its image dims (createBuffer's imageDims) and - a placement matrix - the floats hostAccess wrote"""

    def __init__(self, nbytes, dims=None, host=None):
        self.nbytes, self.dims, self.host = int(nbytes), dims, host

    def make(self, ctx):
        b = ctx.create_buffer(self.nbytes, dims=self.dims, owner="args")
        if self.host is not None:
            b.host_access("writeonly", capi.QUEUE_LOAD, self.host.view(np.uint8)[:self.nbytes])
        return b


def raw(n):
    return B(n)


def img(w, h):
    return B(w * h * 16, dims=(w, h))


def placed(w, h, **kw):
    from test_routes_gpu import m
    return B(36, host=np.asarray(m(w, h, **kw), np.float32).reshape(-1)[:9].copy())


def v210_bytes(w, h):
    return frames.v210_pitch_bytes(w) * h


def loader():
    return [("colMatrix", raw(48)), ("gammaLut", raw(LUT)), ("gamutMatrix", raw(36))]


def saver():
    return [("outColMatrix", raw(48)), ("outGammaLut", raw(LUT))]


class Job:
    def __init__(self, name, kid, source, kernel, gwi, wipg, params, rebuild=None):
        self.name, self.kid, self.source, self.kernel, self.gwi, self.wipg = name, kid, source, kernel, gwi, wipg
        self.params = OrderedDict(params)
        self.rebuild = rebuild  # (w, h) -> the same job at another size (jobs of the even-only formats)


PLANE_NAMES = {1: [""], 2: ["Y", "C"], 3: ["Y", "U", "V"]}


def pack_job(fmt, rd, w=W, h=H):
    f = packfmt.get(fmt)
    try:
        pb = [n for n in f.plane_bytes(w, h) if n]
    except Exception:  # an odd size of an even-only format: the planes of the next even size (the job is refused for its size)
        pb = [n for n in f.plane_bytes(*f.even(w, h)) if n]
    side = "input" if rd else "output"
    p = [(side + s, raw(n)) for s, n in zip(PLANE_NAMES[len(pb)], pb)]
    p.append(("output" if rd else "input", raw(w * h * 16)))
    if f.code_range is not None:
        p.append(("colMatrix", raw(48)))
    p.append(("gammaLut", raw(LUT)))
    p += [("gamutMatrix", raw(36)), ("width", w)] if rd else [("width", w), ("interlace", 0)]
    rows = h // 2 if f.v420 else h
    return Job("%s_%s" % (fmt, "read" if rd else "write"), "K_PACK_READ" if rd else "K_PACK_WRITE", "phaneron:" + fmt, "read" if rd else "write",
               WIPG * rows, WIPG, p, rebuild=(lambda w2, h2: pack_job(fmt, rd, w2, h2)) if f.even_size else None)


def chan_job(out_fmt, w=W, h=H):
    """a cut, a dissolve and a wipe layer: v210, a yuv420p10 decoder frame with its own Loader matrix, an rgba8 graphic, f32 images"""
    f10 = packfmt.get("yuv420p10")
    try:
        pb = f10.plane_bytes(w, h)
    except Exception:
        pb = f10.plane_bytes(*f10.even(w, h))
    p = [("l0In", raw(v210_bytes(w, h))), ("l0Width", w), ("l0Height", h),
         ("l1In", raw(pb[0])), ("l1InU", raw(pb[1])), ("l1InV", raw(pb[2])), ("l1Packing", capi.FORMATS["yuv420p10"]), ("l1ColMatrix", raw(48)),
         ("l1Width", w), ("l1Height", h), ("l1Matrix", placed(w, h, scale_x=0.5, scale_y=0.5)), ("l1Transition", 1), ("l1Mix", 0.25),
         ("l1IncomingIn", raw(v210_bytes(w // 2, h // 2))), ("l1IncomingWidth", w // 2), ("l1IncomingHeight", h // 2),
         ("l1IncomingMatrix", placed(w, h, rotate=0.05)),
         ("l2In", raw(w * h * 4)), ("l2Packing", capi.FORMATS["rgba8"]), ("l2Width", w), ("l2Height", h), ("l2Transition", 2), ("l2Mix", 0.5),
         ("l2IncomingIn", img(w, h)), ("l2MaskIn", img(w, h)), ("l2MaskMatrix", placed(w, h))]
    of = packfmt.get(out_fmt)
    opb = [n for n in of.plane_bytes(w, h) if n]
    p += [("output" + s, raw(n)) for s, n in zip({1: [""], 2: ["", "C"], 3: ["", "U", "V"]}[len(opb)], opb)]
    p.append(("outPacking", capi.FORMATS[out_fmt]))
    p += loader() + [a for a in saver() if of.code_range is not None or a[0] != "outColMatrix"] + [("interlace", 0)]
    return Job("chan_" + out_fmt, "K_CHAN_COMPOSE", "phaneron:chan", "chan_compose_v210_3", [w, h], 0, p,
               rebuild=(lambda w2, h2: chan_job(out_fmt, w2, h2)) if out_fmt == "v210" else None)


def up_job(form):
    p = []
    for i, (lw, lh) in enumerate([(W // 2, H // 2), (W // 4, H // 2)]):
        if form == "packedRgb":
            p += [("l%dIn" % i, raw(lw * lh * 12)), ("l%dWidth" % i, lw), ("l%dHeight" % i, lh)]
        else:
            p.append(("l%dIn" % i, img(lw, lh)))
        if form == "pair":
            p.append(("l%dIn2" % i, img(lw, lh)))
        p.append(("l%dMatrix" % i, placed(W, H, scale_x=2.0, scale_y=2.0)))
    p.append(("output", raw(v210_bytes(W, H))))
    if form == "pair":
        p.append(("output2", raw(v210_bytes(W, H))))
    if form == "packedRgb":
        p.append(("packedRgb", 1))
    return Job("compose_up_" + form, "K_COMPOSE_UP", "phaneron:up", "compose_up_write_v210_2", [W, H], 0, p + saver() + [("interlace", 0)])


def deint_job(fmt):
    p = []
    n = 2 if fmt == "v210" else 1
    pb = [x for x in packfmt.get(fmt).plane_bytes(W, H) if x]
    for i in range(n):
        for which in ("Prev", "Cur", "Next"):
            p += [("l%d%s%s" % (i, which, s), raw(x)) for s, x in zip(["", "U", "V"], pb)]
        p += [("l%dOut0" % i, raw(W * H * 16)), ("l%dOut1" % i, raw(W * H * 16))]
    if fmt != "v210":
        p.append(("packing", capi.FORMATS[fmt]))
    p += loader() + [("tff", 1), ("skipSpatial", 0)]
    return Job("v210_yadif_pair_" + fmt, "K_V210_YADIF_PAIR", "phaneron:yadif", "v210_yadif_pair_%d" % n, [W, H], 0, p)


def compose_v210_job(wipe):
    p = [("l0In", img(W, H)), ("l1In", img(W // 2, H // 2)), ("l1Matrix", raw(36))]
    if wipe:
        p += [("l1WipeIn", raw(W * H * 16)), ("l1WipeMask", raw(W * H * 16))]
    p += [("output", raw(v210_bytes(W, H)))] + saver() + [("interlace", 0)]
    return Job("compose_write_v210" + ("_wipe" if wipe else ""), "K_COMPOSE_V210", "phaneron:compose", "compose_write_v210_2", [W, H], 0, p)


def jobs():
    """the accepted jobs, every kernel id of ph_program.h among them"""
    px = W * H * 16
    out = [pack_job(fmt, rd) for rd in (True, False) for fmt in ("rgba8", "p010", "yuv420p10", "yuv422p8")]
    out.append(Job("v210_read", "K_V210_READ", "phaneron:v210", "read", WIPG * H, WIPG,
                   [("input", raw(v210_bytes(W, H))), ("output", raw(px))] + loader() + [("width", W)]))
    out.append(Job("v210_write", "K_V210_WRITE", "phaneron:v210", "write", WIPG * H, WIPG,
                   [("input", raw(px)), ("output", raw(v210_bytes(W, H))), ("colMatrix", raw(48)), ("gammaLut", raw(LUT)), ("width", W), ("interlace", 0)]))
    out.append(Job("v210_read_batch", "K_V210_READ_BATCH", "phaneron:v210", "v210_read_batch_2", [W, H], 0,
                   [(k, raw(n)) for i in range(2) for k, n in (("l%dIn" % i, v210_bytes(W, H)), ("l%dOut" % i, px))] + loader()))
    window = [("prev", raw(px)), ("cur", raw(px)), ("next", raw(px))]
    out.append(Job("yadif", "K_YADIF", "phaneron:yadif", "yadif", [W, H], 0, [("output", img(W, H))] + window + [("parity", 1), ("tff", 1), ("skipSpatial", 0)]))
    out.append(Job("yadif_pair", "K_YADIF_PAIR", "phaneron:yadif", "yadif_pair", [W, H], 0,
                   [("output0", img(W, H)), ("output1", raw(px))] + window + [("tff", 1), ("skipSpatial", 0)]))
    out += [deint_job("v210"), deint_job("yuv420p")]
    out += [chan_job(f) for f in ("v210", "nv12", "yuv422p8", "rgba8")]
    out += [up_job(form) for form in ("plain", "packedRgb", "pair")]
    out += [compose_v210_job(False), compose_v210_job(True)]
    out.append(Job("transform", "K_TRANSFORM", "phaneron:transform", "transform", [W, H], 0,
                   [("input", img(W // 2, H)), ("output", img(W, H)), ("transformMatrix", raw(32))]))
    out.append(Job("resize", "K_RESIZE", "phaneron:resize", "resize", [W, H], 0,
                   [("input", img(W // 2, H)), ("output", img(W, H)), ("flip", raw(16)), ("scale", 1.5), ("offsetX", 0.25), ("offsetY", -0.25)]))
    out.append(Job("combine", "K_COMBINE", "phaneron:combine", "combine_3", [W, H], 0, [("output", img(W, H))] + [("l%dIn" % i, raw(px)) for i in range(3)]))
    for name, kid, kernel, num in (("dissolve", "K_DISSOLVE", "transition_dissolve", "mix"), ("mixer", "K_MIXER", "mixer", "mix"), ("wipe", "K_WIPE", "wipe", "wipe")):
        out.append(Job(name, kid, "phaneron:" + name, kernel, [W, H], 0, [("output", img(W, H)), ("input0", raw(px)), ("input1", raw(px)), (num, 0.5)]))
    out.append(Job("transition_wipe", "K_TWIPE", "phaneron:transition", "transition_wipe", [W, H], 0,
                   [("output", img(W, H)), ("input0", raw(px)), ("input1", raw(px)), ("maskIn", raw(px))]))
    out.append(Job("rgb_unpack", "K_RGB_UNPACK", "phaneron:rgb", "rgb_unpack", [W, H], 0, [("image", img(W, H))]))
    out.append(Job("fused", "K_FUSED_V210", "phaneron:fused", "fused_v210_combine_2", [W, H], 0,
                   [("l%dIn" % i, raw(v210_bytes(W, H))) for i in range(2)] + [("output", raw(v210_bytes(W, H)))] + loader() + saver()))
    return out


def with_param(job, name, value):
    p = OrderedDict(job.params)
    if value is None:
        del p[name]
    else:
        p[name] = value
    return Job(job.name, job.kid, job.source, job.kernel, job.gwi, job.wipg, p)


def defects(job):
    """(case id, job, must it be refused?) for the job itself and every job derived from it by one defect"""
    yield job.name + "/accepted", job, False
    for k, v in job.params.items():
        yield "%s/-%s" % (job.name, k), with_param(job, k, None), None
        if isinstance(v, B):
            if v.dims is None or v.nbytes > v.dims[0] * v.dims[1] * 16:  # (createBuffer itself refuses an image smaller than its dims)
                yield "%s/short:%s" % (job.name, k), with_param(job, k, B(v.nbytes - 1, v.dims, v.host)), True
            yield "%s/number:%s" % (job.name, k), with_param(job, k, 1), True
            if v.dims is not None:
                yield "%s/plain:%s" % (job.name, k), with_param(job, k, B(v.nbytes)), None  # (a channel source without dims is a v210 frame)
            if v.host is not None:
                yield "%s/nohost:%s" % (job.name, k), with_param(job, k, B(v.nbytes)), True
        else:
            yield "%s/buffer:%s" % (job.name, k), with_param(job, k, B(16)), None
        if k.lower().endswith("packing"):
            for bad in [-1, len(capi.FORMATS)] + ([capi.FORMATS[f] for f in packfmt.NOT_CHAN_OUT] if k == "outPacking" else []):
                yield "%s/%s=%d" % (job.name, k, bad), with_param(job, k, bad), True
    zero = [0] * len(job.gwi) if isinstance(job.gwi, list) else 0
    yield job.name + "/globalWorkItems=0", Job(job.name, job.kid, job.source, job.kernel, zero, job.wipg, job.params), None
    if job.wipg:
        yield job.name + "/workItemsPerGroup=0", Job(job.name, job.kid, job.source, job.kernel, job.gwi, 0, job.params), True
    if job.rebuild:
        yield job.name + "/odd-width", job.rebuild(W + 1, H), None
        yield job.name + "/odd-height", job.rebuild(W, H + 1), None


def check(ctx, job, made=None):
    """[return code, ph_last_error text] of the job under ph_check_program; `made`: buffers of the accepted job to use where the specs are the same"""
    prog = ctx.create_program(job.source, job.kernel, job.gwi, job.wipg)
    own, params = [], OrderedDict()
    for k, v in job.params.items():
        if isinstance(v, B):
            if made is not None and made.get(k, (None, None))[0] is v:
                params[k] = made[k][1]
            else:
                params[k] = v.make(ctx)
                own.append(params[k])
        else:
            params[k] = v
    try:
        ctx.run_program(prog, params, check_only=True)
        got = [0, ""]
    except capi.PhaneronError as e:
        m = re.match(r"libphaneron_hip error (-?\d+): (.*)$", str(e), re.S)
        got = [int(m.group(1)), m.group(2)]
    for b in own:
        b.release()
    prog.destroy()
    return got


def run_cases(ctx, job):
    made = {k: (v, v.make(ctx)) for k, v in job.params.items() if isinstance(v, B)}
    ctx.wait(capi.QUEUE_LOAD)
    out, wrong = OrderedDict(), []
    for cid, j, refused in defects(job):
        got = check(ctx, j, made if j.rebuild is None or j is job else None)
        print(cid, got)
        # what a derived job must do whatever the text: the job itself is accepted, a job with a defect no argument list tolerates is not
        if refused is not None and (got[0] != 0) != refused:
            wrong.append((cid, got))
        out[cid] = got
    for _, b in made.values():
        b.release()
    assert not wrong, wrong
    return out


JOBS = jobs()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def recorded():
    with open(RECORD) as f:
        return json.load(f)


def test_every_kernel_id_has_a_job_and_the_record_holds_exactly_the_derived_cases():
    with open(os.path.join(HERE, "..", "phaneron_amd", "csrc", "ph_program.h")) as f:
        ids = set(re.findall(r"^\s*(K_\w+)", f.read(), re.M))
    assert len(ids) == 20 and {j.kid for j in JOBS} == ids
    assert len({j.name for j in JOBS}) == len(JOBS)
    derived = [cid for j in JOBS for cid, _, _ in defects(j)]
    assert len(set(derived)) == len(derived)
    want = set(recorded())
    assert set(derived) == want, (sorted(set(derived) - want), sorted(want - set(derived)))


@pytest.mark.parametrize("job", JOBS, ids=[j.name for j in JOBS])
def test_codes_and_texts_are_the_recorded_ones(ctx, job):
    want = recorded()
    got = run_cases(ctx, job)
    bad = {cid: (g, want.get(cid)) for cid, g in got.items() if want.get(cid) != g}
    assert not bad, bad


# ---- the accepted jobs, run: the by-name call writes what the typed call writes ---------------------------------------------------
# (test_boundary_gpu.py, test_packfmt_gpu.py and the node tests run the other programs by name against the oracle)

def fill(ctx, job, seed):
    """buffers for a job's arguments with data in them: legal v210 words, random bytes, images in [0, 1], real Loader / Saver tables"""
    rng = np.random.default_rng(seed)
    table = {"colMatrix": capi.ycbcr2rgb_matrix("709"), "gammaLut": capi.gamma2linear_lut("709"), "gamutMatrix": capi.rgb2rgb_matrix("709", "2020"),
             "outColMatrix": capi.rgb2ycbcr_matrix("2020"), "outGammaLut": capi.linear2gamma_lut("2020")}
    made = OrderedDict()
    for k, v in job.params.items():
        if not isinstance(v, B):
            made[k] = v
            continue
        b = ctx.create_buffer(v.nbytes, dims=v.dims, owner="args")
        if v.host is not None:
            data = v.host
        elif k in table:
            data = np.zeros(v.nbytes // 4, np.float32)
            data[:table[k].size] = np.asarray(table[k], np.float32).reshape(-1)
        elif k.endswith("ColMatrix"):
            data = capi.ycbcr2rgb_matrix("709")
        elif v.dims is not None or v.nbytes == W * H * 16 or ("packedRgb" in job.params and re.match(r"l\dIn", k)):
            data = rng.random(v.nbytes // 4, dtype=np.float32)
        else:  # (wire frames: any bytes are a frame)
            data = rng.integers(0, 256, v.nbytes, dtype=np.uint8)
        b.host_access("writeonly", capi.QUEUE_LOAD, data)
        made[k] = b
    ctx.wait(capi.QUEUE_LOAD)
    return made


def fetch(ctx, b):
    b.host_access("readonly", capi.QUEUE_UNLOAD)
    return b.host(np.uint8).copy()


class Dev:
    """a Buffer's device memory as the typed calls take it"""

    def __init__(self, b):
        self.b = b

    def data_ptr(self):
        return self.b.device_ptr()


def outputs(job):
    return [k for k in job.params if re.match(r"output|l\dOut", k)]


def typed_chan(ctx, a, job):
    fmt = {v: k for k, v in capi.FORMATS.items()}[a["outPacking"]]
    d = lambda k: Dev(a[k])
    m9 = lambda k: job.params[k].host[:9]
    w2, h2 = W // 2, H // 2
    layers = [dict(src=(d("l0In"), W, H, None)),
              dict(src=((d("l1In"), d("l1InU"), d("l1InV")), W, H, m9("l1Matrix"), "yuv420p10", d("l1ColMatrix")), transition="dissolve", mix=0.25,
                   incoming=(d("l1IncomingIn"), w2, h2, m9("l1IncomingMatrix"))),
              dict(src=(d("l2In"), W, H, None, "rgba8"), transition="wipe", mix=0.5, incoming=(d("l2IncomingIn"), W, H, None, "rgba"),
                   mask=(d("l2MaskIn"), W, H, m9("l2MaskMatrix"), "rgba"))]
    dst = [d(k) for k in outputs(job)]
    ctx.chan_compose_v210(layers, dst[0] if fmt == "v210" else tuple(dst), W, H, 0, d("colMatrix"), d("gammaLut"), d("gamutMatrix"),
                          d("outColMatrix") if "outColMatrix" in a else None, d("outGammaLut"), **({} if fmt == "v210" else {"out_fmt": fmt}))


def typed_up(ctx, a, job):
    d = lambda k: Dev(a[k])
    rgb = "packedRgb" in a
    sizes = [(W // 2, H // 2), (W // 4, H // 2)]
    sets = [[(d("l%dIn%s" % (i, s)), lw, lh, job.params["l%dMatrix" % i].host[:9]) for i, (lw, lh) in enumerate(sizes)] for s in (["", "2"] if "output2" in a else [""])]
    if len(sets) == 2:
        ctx.compose_up_write_v210_pair(sets[0], sets[1], d("output"), d("output2"), W, H, 0, d("outColMatrix"), d("outGammaLut"))
    else:
        ctx.compose_up_write_v210(sets[0], d("output"), W, H, 0, d("outColMatrix"), d("outGammaLut"), rgb=rgb)


def typed_compose_v210(ctx, a, job):
    d = lambda k: Dev(a[k])
    layers = [(d("l0In"), W, H, None), (d("l1In"), W // 2, H // 2, d("l1Matrix"))]
    if "l1WipeIn" in a:
        ctx.compose_wipe_write_v210(layers, [None, (d("l1WipeIn"), d("l1WipeMask"))], d("output"), W, H, 0, d("outColMatrix"), d("outGammaLut"))
    else:
        ctx.compose_write_v210(layers, d("output"), W, H, 0, d("outColMatrix"), d("outGammaLut"))


TYPED = {"K_CHAN_COMPOSE": typed_chan, "K_COMPOSE_UP": typed_up, "K_COMPOSE_V210": typed_compose_v210}
RUN = [j for j in JOBS if j.kid in TYPED]


@pytest.mark.parametrize("job", RUN, ids=[j.name for j in RUN])
def test_an_accepted_job_writes_what_the_typed_call_writes(ctx, job):
    a = fill(ctx, job, 4200 + JOBS.index(job))
    if job.kid == "K_COMPOSE_V210":  # (this program reads its placement on the device: a 3 x 3 matrix in the buffer)
        a["l1Matrix"].host_access("writeonly", capi.QUEUE_LOAD, np.asarray(capi.transform_matrix(W, H, scale_x=0.5, scale_y=0.5), np.float32))
        ctx.wait(capi.QUEUE_LOAD)
    prog = ctx.create_program(job.source, job.kernel, job.gwi, job.wipg)
    got = []
    for by_name in (True, False):
        for k in outputs(job):
            a[k].host_access("writeonly", capi.QUEUE_LOAD, np.full(a[k].nbytes, packfmt.POISON, np.uint8))
        ctx.wait(capi.QUEUE_LOAD)
        if by_name:
            ctx.run_program(prog, a)
        else:
            TYPED[job.kid](ctx, a, job)
        ctx.wait()
        got.append([fetch(ctx, a[k]) for k in outputs(job)])
        ctx.wait(capi.QUEUE_UNLOAD)
    for k, x, y in zip(outputs(job), *got):
        assert not (x == packfmt.POISON).all(), k
        assert np.array_equal(x, y), k
    prog.destroy()
    for v in a.values():
        if isinstance(v, capi.Buffer):
            v.release()


if __name__ == "__main__":  # the recorder: every derived case as the loaded library answers it
    with capi.Context(0) as c:
        cases = OrderedDict()
        for job_ in JOBS:
            cases.update(run_cases(c, job_))
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else RECORD, "w") as f_:
        json.dump(cases, f_, indent=0, sort_keys=True)
        f_.write("\n")
    print("%d cases of %d jobs recorded from %s" % (len(cases), len(JOBS), capi.LIB_PATH))
