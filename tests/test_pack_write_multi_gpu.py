"""GPU tests (-m gpu) of ph_pack_write_multi: one f32 RGBA image packed for up to four consumers in one call.  The contract is "exactly
the n_out calls of ph_pack_write", so every case is compared byte for byte - the bytes a call must leave alone included
(packfmt.POISON) - with the oracle's writers (packfmt.oracle_write; the 10-bit 4:2:0 formats through fmt10) AND with the separate
ph_pack_write calls into equally poisoned planes.  The trace says which launches made the frames: one "pack_write_multi x<k>" per
registered table, the outputs the shared kernel does not take under ph_pack_write's own names."""
import ctypes

import numpy as np
import pytest

import frames
import packfmt
from phaneron_amd import capi

pytestmark = pytest.mark.gpu

ALL = list(packfmt.NAMES)
PAIRS = [("v210", f) for f in ALL if f != "v210"]
QUAD_10 = ("yuv420p10", "p010", "v210", "rgba8")
QUAD_8 = ("yuv422p8", "yuv420p", "nv12", "bgra8")
SAME = ("yuv422p10", "yuv422p10")
WIDTHS = [48, 96, 192, 80, 8, 22, 50, 2]
HEIGHTS = [2, 4, 6, 10, 7]


def O(fmt, interlace=0, spec="709", table="registered"):
    """an output: table "registered" (the spec's shared table), "own" (a registered copy under its own pointer), "plain" (not registered)"""
    return dict(fmt=fmt, interlace=interlace, spec=spec, table=table)


_tables = {}


def device_writer(o):
    """(matrix tensor or None, table tensor) of an output"""
    import hip_harness as hh
    cm, lut = hh.ColourParams.fmt_writer(o["fmt"], o["spec"])
    if o["table"] != "registered":
        key = (o["spec"], o["table"])
        if key not in _tables:
            host = capi.linear2gamma_lut(o["spec"])
            _tables[key] = hh.dev(host)
            if o["table"] == "own":
                hh.ctx().register_lut(_tables[key], host)
        lut = _tables[key]
    return cm, lut


def defined(outs, w, h):
    """the outputs of a case whose format is defined at w x h (the 10-bit 4:2:0 frames: even sizes only)"""
    return [o for o in outs if not (packfmt.get(o["fmt"]).even_size and ((w | h) & 1))]


def takes(o, w):
    """does the shared kernel take the output at this width?"""
    f = packfmt.get(o["fmt"])
    return o["table"] != "plain" and not (o["fmt"] == "v210" and w % 48) and not (f.planar and w % 8)


def expected_route(outs, w, alone, lds=True):
    """the launches of a call, from the rule in include/phaneron_hip.h; alone[i]: what ph_pack_write's own launch of output i is called"""
    route, seen = [], []
    for o in outs:
        key = (o["spec"], o["table"])
        if key in seen:
            continue
        seen.append(key)
        group = [i for i, p in enumerate(outs) if (p["spec"], p["table"]) == key]
        share = [i for i in group if lds and takes(outs[i], w)]
        if len(share) < 2:
            share = []
        route += [alone[i] for i in group if i not in share]
        if share:
            route.append("pack_write_multi x%d" % len(share))
    return "+".join(route)


def as_bytes(planes):
    return [np.ascontiguousarray(np.asarray(p).reshape(-1)).view(np.uint8) for p in planes]


def run(w, h, outs, rgba, passes=1, oracle=True, lds=True):
    """One ph_pack_write_multi call (passes: a list of per-output interlace lists run one after the other into the same planes) against
    the separate ph_pack_write calls and the oracle; returns the traced route of the last call and the names of the separate launches."""
    import hip_harness as hh
    k = hh.ctx()
    d_rgba = hh.dev(rgba)
    fmts = [packfmt.get(o["fmt"]) for o in outs]
    recipes = [device_writer(o) for o in outs]
    multi = [[hh.dev(p) for p in f.poisoned(w, h)] for f in fmts]
    apart = [[hh.dev(p) for p in f.poisoned(w, h)] for f in fmts]
    want = [as_bytes(f.poisoned(w, h)) for f in fmts]
    passes = passes if isinstance(passes, list) else [[o["interlace"] for o in outs]]
    route, alone = None, []
    for ils in passes:
        call = [dict(fmt=o["fmt"], planes=d, interlace=il, wr_cm=rc[0], wr_lut=rc[1]) for o, d, il, rc in zip(outs, multi, ils, recipes)]
        with capi.trace() as t:
            k.pack_write_multi(d_rgba, call, w, h)
        route, alone = t.route, []
        for o, d, il, rc in zip(outs, apart, ils, recipes):
            with capi.trace() as t1:
                k.pack_write(o["fmt"], d_rgba, d, w, h, il, rc[0], rc[1])
            alone.append(t1.route)
        if oracle:
            for i, (o, f, il) in enumerate(zip(outs, fmts, ils)):
                cm, lut = f.oracle_writer(o["spec"])
                want[i] = as_bytes(f.oracle_write(rgba, w, h, il, cm, lut, [p.view(np.uint32) if o["fmt"] == "v210" else p for p in want[i]]))
    for i, o in enumerate(outs):
        for pl in range(len(multi[i])):
            got, sep = as_bytes([hh.host(multi[i][pl])])[0], as_bytes([hh.host(apart[i][pl])])[0]
            what = "%dx%d output %d (%s, fields %s) plane %d" % (w, h, i, o["fmt"], [p[i] for p in passes], pl)
            bad = np.flatnonzero(got != sep)
            assert bad.size == 0, "%s: %d of %d bytes differ from the separate ph_pack_write call, first at %d" % (what, bad.size, got.size, bad[0])
            if oracle:
                bad = np.flatnonzero(got != want[i][pl])
                assert bad.size == 0, "%s: %d of %d bytes differ from the oracle, first at %d" % (what, bad.size, got.size, bad[0])
    return route, alone, multi


def image(w, h, seed):
    return frames.rgba_specials(w, h, seed) if seed & 1 else frames.rgba_random(w, h, seed, -0.05, 1.05)


@pytest.mark.parametrize("fmt", ALL)
def test_one_output_is_ph_pack_write(fmt):
    for w in WIDTHS:
        for h in (4, 7):
            outs = defined([O(fmt)], w, h)
            if outs:
                route, alone, _ = run(w, h, outs, image(w, h, 11 + w))
                assert route == alone[0] and "multi" not in route, (w, h, route, alone)


@pytest.mark.parametrize("spec", ["709", "2020"])
@pytest.mark.parametrize("w", WIDTHS)
def test_pairs_and_quadruples(w, spec):
    cases = PAIRS + [QUAD_10, QUAD_8, SAME]
    for n, case in enumerate(cases):
        for h in HEIGHTS:
            outs = defined([O(f, spec=spec) for f in case], w, h)
            if not outs:
                continue
            route, alone, _ = run(w, h, outs, image(w, h, 100 * n + h + (spec == "2020")))
            assert route == expected_route(outs, w, alone), (case, w, h, route, alone)
            share = [o for o in outs if takes(o, w)]
            assert route.count("pack_write_multi") == (1 if len(share) > 1 else 0), (case, w, h, route)


MODES = {"all-0": (0, 0, 0, 0), "all-1": (1, 1, 1, 1), "all-3": (3, 3, 3, 3), "mixed": (0, 1, 3, 1)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", [QUAD_10, QUAD_8], ids=["quad10", "quad8"])
def test_field_modes(case, mode):
    import hip_harness as hh
    for w, h in ((96, 10), (48, 6), (96, 4), (48, 7)):
        outs = defined([O(f, il) for f, il in zip(case, MODES[mode])], w, h)
        if not outs:
            continue
        route, _, planes = run(w, h, outs, image(w, h, 7 * h + 1))
        assert route == "pack_write_multi x%d" % len(outs), route
        for o, d in zip(outs, planes):  # the rows of the other field (and the unpaired last line of a 4:2:0 frame) keep the poison
            f = packfmt.get(o["fmt"])
            luma = as_bytes([hh.host(d[0])])[0].reshape(h, -1)
            for r in f.rows_untouched(h, o["interlace"]):
                assert (luma[r] == packfmt.POISON).all(), "%s field %d: row %d of %d was written" % (o["fmt"], o["interlace"], r, h)
            if f.v420 and o["interlace"] == 0 and h & 1:
                assert (luma[h - 1] == packfmt.POISON).all(), "%s: the unpaired last line was written" % o["fmt"]
            if f.v420 and h % 2 == 0:  # every chroma row is written, whatever the mode (the oracle pins from which line)
                chroma = as_bytes([hh.host(d[1])])[0].reshape(h // 2, -1)
                assert (chroma != packfmt.POISON).any(axis=1).all(), "%s field %d: a chroma row was left unwritten" % (o["fmt"], o["interlace"])


@pytest.mark.parametrize("case", [QUAD_10, QUAD_8], ids=["quad10", "quad8"])
def test_field_1_then_field_3_into_the_same_planes(case):
    for w, h in ((96, 10), (48, 4)):
        outs = [O(f) for f in case]
        route, _, _ = run(w, h, outs, image(w, h, 31), passes=[[1] * 4, [3] * 4])
        assert route == "pack_write_multi x4", route


def test_two_tables_are_two_launches_in_output_order():
    w, h = 96, 6
    outs = [O("v210", spec="709"), O("rgba8", spec="sRGB"), O("yuv422p8", spec="709"), O("bgra8", spec="sRGB")]
    route, alone, _ = run(w, h, outs, image(w, h, 41))
    assert route == "pack_write_multi x2+pack_write_multi x2" == expected_route(outs, w, alone), route
    # an output alone with its table is split off; a registered copy of the same table is another table
    outs = [O("v210"), O("rgba8", table="own"), O("p010")]
    route, alone, _ = run(w, h, outs, image(w, h, 43))
    assert route == "pack_write_multi x2+" + alone[1] == expected_route(outs, w, alone), route


def test_without_an_lds_table_only_the_present_routes_appear():
    import hip_harness as hh
    w, h = 96, 6
    outs = [O("v210"), O("p010"), O("rgba8")]
    hh.ctx().set_option("lds_lut", False)
    try:
        route, alone, _ = run(w, h, outs, image(w, h, 51), lds=False)
    finally:
        hh.ctx().set_option("lds_lut", True)
    assert route == "+".join(alone) and "multi" not in route, (route, alone)
    outs = [O(f, table="plain") for f in ("v210", "p010", "rgba8")]
    route, alone, _ = run(w, h, outs, image(w, h, 53))
    assert route == "+".join(alone) and "multi" not in route, (route, alone)


def test_a_v210_line_tail_is_split_off_beside_one_shared_launch():
    w, h = 80, 6
    outs = [O("v210"), O("p010"), O("rgba8")]
    route, alone, _ = run(w, h, outs, image(w, h, 61))
    assert route == alone[0] + "+pack_write_multi x2", (route, alone)
    w = 50  # planar split off, the two packed-RGB outputs shared
    outs = [O("rgba8"), O("yuv422p8"), O("bgra8", 3)]
    route, alone, _ = run(w, h, outs, image(w, h, 63))
    assert route == alone[1] + "+pack_write_multi x2", (route, alone)


def test_full_size_equals_the_three_separate_calls():
    w, h = 3840, 2160
    outs = [O("v210", spec="2020"), O("p010", spec="2020"), O("rgba8", spec="2020")]
    route, _, _ = run(w, h, outs, frames.rgba_random(w, h, 71, -0.05, 1.05), oracle=False)
    assert route == "pack_write_multi x3", route


# ---- refusals: decided before anything is launched ----------------------------------------------------------------------------------
def test_every_refusal_leaves_every_plane_alone():
    import hip_harness as hh
    k = hh.ctx()
    w, h = 48, 4
    d_rgba = hh.dev(image(w, h, 81))
    fmts = ["v210", "yuv422p8", "p010", "rgba8"]
    planes = [[hh.dev(p) for p in packfmt.get(f).poisoned(w, h)] for f in fmts]
    recipes = [device_writer(O(f)) for f in fmts]
    good = [dict(fmt=f, planes=list(d), interlace=0, wr_cm=rc[0], wr_lut=rc[1]) for f, d, rc in zip(fmts, planes, recipes)]

    def with_(i, **kw):
        outs = [dict(o) for o in good]
        outs[i].update(kw)
        return outs

    cases = [
        ("NULL in", None, good, w, h, "NULL"),
        ("no outputs", d_rgba, [], w, h, "1..4 outputs"),
        ("five outputs", d_rgba, good + [good[0]], w, h, "1..4 outputs"),
        ("unknown format", d_rgba, with_(1, fmt=99), w, h, "unknown format 99"),
        ("interlace 2", d_rgba, with_(3, interlace=2), w, h, "interlace must be 0, 1 or 3"),
        ("missing plane", d_rgba, with_(1, planes=[planes[1][0], None, planes[1][2]]), w, h, "plane 1 is NULL"),
        ("missing first plane", d_rgba, with_(0, planes=[None]), w, h, "plane 0 is NULL"),
        ("missing matrix", d_rgba, with_(2, wr_cm=None), w, h, "colMatrix"),
        ("missing table", d_rgba, with_(3, wr_lut=None), w, h, "gamma LUT"),
        ("odd width", d_rgba, good, w - 1, h, "needs an even width and height"),
        ("odd height", d_rgba, good, w, h - 1, "needs an even width and height"),
        ("same first plane", d_rgba, with_(3, planes=[planes[0][0]]), w, h, "name the same plane"),
        ("width 0", d_rgba, good, 0, h, "NULL/zero"),
    ]
    for what, src, outs, cw, ch, needle in cases:
        with pytest.raises(capi.PhaneronError, match=needle) as e:
            k.pack_write_multi(src, outs, cw, ch)
        assert "error -1:" in str(e.value), (what, str(e.value))
    arr = capi.Context._chan_outputs(good)
    fn = capi.lib().ph_pack_write_multi
    assert fn(None, capi.QUEUE_PROCESS, ctypes.c_void_p(d_rgba.data_ptr()), 4, arr, w, h) == -1, "a NULL context"
    assert fn(k.h, capi.QUEUE_PROCESS, ctypes.c_void_p(d_rgba.data_ptr()), 4, None, w, h) == -1, "NULL outputs"
    assert fn(k.h, 7, ctypes.c_void_p(d_rgba.data_ptr()), 4, arr, w, h) == -1, "a queue that does not exist"
    k.pack_write_multi(d_rgba, good, w, 0)  # height 0: PH_OK, nothing written
    for f, d in zip(fmts, planes):
        for pl, p in enumerate(d):
            assert (as_bytes([hh.host(p)])[0] == packfmt.POISON).all(), "a refused call wrote %s plane %d" % (f, pl)


# ---- by name: pack_write_multi_<n> ---------------------------------------------------------------------------------------------------
W, H = 96, 6


@pytest.fixture
def by_name():
    from test_chan_multi_gpu import ByName
    b = ByName(W, H)
    yield b
    b.close()


def named_outputs(b, fmts, interlace):
    """the arguments of the outputs and, per output, its plane buffers"""
    params, planes = {}, []
    for k, (fmt, il) in enumerate(zip(fmts, interlace)):
        f = packfmt.get(fmt)
        num = str(k) if k else ""
        bufs = [b.upload(p, svm="coarse") for p in f.poisoned(W, H)]
        planes.append(bufs)
        names = ["output" + num] if len(bufs) == 1 else ["output" + num, "output%sC" % num] if len(bufs) == 2 else ["output" + num, "output%sU" % num, "output%sV" % num]
        params.update(dict(zip(names, bufs)))
        params["out%sPacking" % num] = capi.FORMATS[fmt]
        params["interlace" + num] = il
        params["out%sGammaLut" % num] = b.recipe["outGammaLut"]
        if f.code_range is not None:
            params["out%sColMatrix" % num] = b.upload(capi.rgb2ycbcr_matrix("709", *f.code_range))
    return params, planes


def typed_bytes(rgba, fmts, interlace):
    """what the typed call makes of the same image (its own bytes are pinned above)"""
    import hip_harness as hh
    d_rgba = hh.dev(rgba)
    dst = [[hh.dev(p) for p in packfmt.get(f).poisoned(W, H)] for f in fmts]
    outs = [dict(fmt=f, planes=d, interlace=il, wr_cm=device_writer(O(f))[0], wr_lut=device_writer(O(f))[1]) for f, d, il in zip(fmts, dst, interlace)]
    hh.ctx().pack_write_multi(d_rgba, outs, W, H)
    return [[as_bytes([hh.host(p)])[0] for p in d] for d in dst]


@pytest.mark.parametrize("fmts,interlace", [(("p010",), (0,)), (("v210", "yuv420p10"), (0, 0)), (("v210", "p010", "rgba8"), (1, 0, 3)), (QUAD_8, (0, 1, 3, 1))],
                         ids=["1", "2", "3", "4"])
def test_by_name_equals_the_typed_call(by_name, fmts, interlace):
    b = by_name
    rgba = image(W, H, 91)
    want = typed_bytes(rgba, fmts, interlace)
    src = b.upload(rgba, svm="coarse")
    name = "pack_write_multi_%d" % len(fmts)
    prog = b.ctx.create_program("phaneron:pack", name, [W, H])
    assert prog.kernel() == name
    # alone
    params, planes = named_outputs(b, fmts, interlace)
    params.update(input=src, width=W)
    b.ctx.wait(capi.QUEUE_LOAD)
    assert b.ctx.run_program(prog, params, check_only=True) is None
    with capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert ("pack_write_multi x%d" % len(fmts) in t.route) == (len(fmts) > 1), t.route
    for i, d in enumerate(planes):
        for pl, p in enumerate(d):
            assert np.array_equal(b.read(p), want[i][pl]), "%s alone: output %d plane %d" % (name, i, pl)
    # between two other jobs of one ph_run_programs call
    params, planes = named_outputs(b, fmts, interlace)
    params.update(input=src, width=W)
    wipg = frames.v210_pitch_pixels(W) // 48
    wr = b.ctx.create_program("phaneron:v210", "write", wipg * H, wipg)
    sdi = [b.upload(packfmt.get("v210").poisoned(W, H)[0], svm="coarse") for _ in range(2)]
    around = [dict(input=src, output=s, width=W, interlace=0, colMatrix=b.recipe["outColMatrix"], gammaLut=b.recipe["outGammaLut"]) for s in sdi]
    b.ctx.wait(capi.QUEUE_LOAD)
    with capi.trace() as t:
        b.ctx.run_programs([(wr, around[0]), (prog, params), (wr, around[1])])
    b.ctx.wait()
    assert t.route.startswith("v210_write") and t.route.endswith("v210_write_lds") and t.route.count("v210_write_lds") >= 2, t.route
    sdi_want = typed_bytes(rgba, ("v210",), (0,))[0][0]
    for s in sdi:
        assert np.array_equal(b.read(s), sdi_want), "the jobs around the several-outputs job"
    for i, d in enumerate(planes):
        for pl, p in enumerate(d):
            assert np.array_equal(b.read(p), want[i][pl]), "%s in ph_run_programs: output %d plane %d" % (name, i, pl)
    prog.destroy()
    wr.destroy()


def test_by_name_defects_name_their_argument_and_check_says_the_same(by_name):
    b = by_name
    fmts, interlace = ("v210", "p010", "yuv420p10"), (0, 0, 0)  # (outPacking 8 and 7: accepted by this program)
    params, planes = named_outputs(b, fmts, interlace)
    params.update(input=b.upload(image(W, H, 93), svm="coarse"), width=W)
    b.ctx.wait(capi.QUEUE_LOAD)
    prog = b.ctx.create_program("", "pack_write_multi_3", [W, H])
    assert b.ctx.run_program(prog, params, check_only=True) is None
    defects = [({k: v for k, v in params.items() if k != "out1GammaLut"}, "'out1GammaLut'"), (dict(params, out1Packing=99), "'out1Packing'"),
               (dict(params, output2=params["output"]), "'output2'"), ({k: v for k, v in params.items() if k != "width"}, "'width'"),
               ({k: v for k, v in params.items() if k != "input"}, "'input'"), ({k: v for k, v in params.items() if k != "output1C"}, "'output1C'"),
               (dict(params, width=W - 48), "globalWorkItems"), (dict(params, interlace1=2), "interlace must be 0, 1 or 3")]
    for job, needle in defects:
        seen = []
        for check_only in (True, False):
            if needle.startswith("interlace") and check_only:  # (the typed call's own refusal: a launch's, not an argument's)
                continue
            with pytest.raises(capi.PhaneronError) as e:
                b.ctx.run_program(prog, job, check_only=check_only)
            seen.append(str(e.value))
        assert all(s == seen[0] for s in seen) and needle in seen[0], seen
    for d in planes:
        for p in d:
            assert (b.read(p) == packfmt.POISON).all(), "a refused job wrote"
    prog.destroy()
    # the channel kernel's programs still refuse the two formats
    chan = b.ctx.create_program("", "chan_compose_v210_1", [W, H])
    vin = b.upload(frames.v210_random(W, H, 95), svm="coarse")
    for packing in (7, 8):
        job = dict(b.recipe, l0In=vin, outPacking=packing, output=planes[1][0], outputC=planes[1][1], outputU=planes[2][1], outputV=planes[2][2], interlace=0)
        with pytest.raises(capi.PhaneronError, match="does not write"):
            b.ctx.run_program(chan, job, check_only=True)
    chan.destroy()
