"""GPU tests (-m gpu): the three entries that follow the context option "up_v210_tails" run with the option at 1 and every source plane and
every output plane between guard bands (tests/guard.py), at 104 x 6 (the second wave step holds cleared slots only: its lanes lie beyond
the line's pixels) and 128 x 5 (an odd height: the last row is its own partner).  A store outside a plane of the header's size damages a
guard and guard.check() names it; a load outside a source plane - a tap where the border colour belongs - brings a value (0xFF codes, NaN
floats) that changes the frame, which is compared with the one made from plain buffers.  The option is put back to 0."""
import numpy as np
import pytest

import frames
import guard
from test_chan_gpu import Src, colour, m
from test_chan_multi_gpu import out, poisoned, writer
from test_clip_multi_gpu import check_clip
from test_clip_multi_guard_gpu import guarded_source
import test_up_out_gpu as up_out

pytestmark = pytest.mark.gpu

SHAPES = [(104, 6, 40, 2, ["v210", "yuv420p", "rgba8"]), (128, 5, 48, 2, ["yuv422p8", "v210", "bgra8"])]


@pytest.fixture
def tails():
    import hip_harness as hh
    k = hh.ctx()
    k.set_option("up_v210_tails", 1)
    try:
        yield k
    finally:
        k.set_option("up_v210_tails", 0)
        guard.reset()


def guarded_outputs(outs, w, h, tag=""):
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    dst = [[guard.dev(p, "dst", pitch=p.nbytes // h, label="%s%s plane %d" % (tag, o["fmt"], i)) for i, p in enumerate(poisoned(o["fmt"], w, h))] for o in outs]
    return dst, [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]


def same_as_plain(dst, plain, what):
    import hip_harness as hh
    for i, d in enumerate(dst):
        for pl, p in enumerate(d):
            assert np.array_equal(hh.host(p, np.uint8), plain[i][pl]), "%s: output %d plane %d differs from the frame made from plain buffers" % (what, i, pl)


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_clip_compose_multi_between_guards(tails, shape):
    import torch
    from phaneron_amd import capi
    w, h, sw, sh, fmts = SHAPES[shape]
    # (an inset that leaves a border on the left and runs off the frame on the right: the lanes beyond the line have taps inside the clip's columns)
    for kw in (dict(), dict(scale_x=0.75, scale_y=1.0, offset_x=0.2)):
        src = Src.random("yuv422p10", sw, sh, 8300 + shape, m(w, h, **kw))
        outs = [out(f) for f in fmts]
        rd_d = colour("709", "709")[2]
        route, plain = check_clip([dict(src=src)], w, h, outs, "%dx%d %r, plain buffers" % (w, h, kw), separate=False)
        assert route == "clip_up_multi_t<rgb>x3", route
        guard.reset()
        dst, outputs = guarded_outputs(outs, w, h)
        with capi.trace() as t:
            tails.clip_compose_multi([dict(src=guarded_source(src), transition="cut", mix=0.0)], outputs, w, h, *rd_d)
        tails.wait()
        torch.cuda.synchronize()
        assert t.route == route, t.route
        n_src, n_dst = guard.check()
        assert n_src == len(src.data) + int(src.own_matrix()) and n_dst == sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
        same_as_plain(dst, plain, "%dx%d %r" % (w, h, kw))


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_clip_compose_batch_out_between_guards(tails, shape):
    import torch
    from phaneron_amd import capi
    w, h, sw, sh, fmts = SHAPES[shape]
    srcs = [Src.random(f, sw, sh, 8400 + 10 * shape + j, m(w, h)) for j, f in enumerate(["yuv422p10", "yuv422p8", "yuv420p"])]
    outs = [out(f) for f in fmts]
    rd_d = colour("709", "709")[2]
    plain = [check_clip([dict(src=s)], w, h, outs, "job %d from plain buffers" % j, separate=False)[1] for j, s in enumerate(srcs)]
    guard.reset()
    jobs, dsts = [], []
    for j, s in enumerate(srcs):
        dst, outputs = guarded_outputs(outs, w, h, "job %d " % j)
        jobs.append(([dict(src=guarded_source(s), transition="cut", mix=0.0)], outputs))
        dsts.append(dst)
    with capi.trace() as t:
        tails.clip_compose_batch_out(jobs, w, h, *rd_d)
    tails.wait()
    torch.cuda.synchronize()
    assert t.route == "clip_up_multi_t<rgb>x3j3", t.route
    n_src, n_dst = guard.check()
    assert n_src == sum(len(s.data) + int(s.own_matrix()) for s in srcs) and n_dst == 3 * sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
    for j, dst in enumerate(dsts):
        same_as_plain(dst, plain[j], "job %d" % j)


@pytest.mark.parametrize("rgb", [False, True], ids=["rgba", "packed-rgb"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_compose_up_write_multi_between_guards(tails, shape, rgb):
    import torch
    from phaneron_amd import capi
    w, h, sw, sh, fmts = SHAPES[shape]
    sets = [up_out.images(w, h, [(sw, sh, dict()), (sw // 2, 1, dict(scale_x=0.5, scale_y=0.5, offset_x=0.3, offset_y=-0.1))], rgb, 8500 + 10 * j) for j in range(2)]
    outs = [out(f) for f in fmts]
    route, plain = up_out.check(sets, w, h, outs, "%dx%d, plain buffers" % (w, h), rgb)
    assert route == "compose_up_multi_t<%s>x3j2" % ("rgb" if rgb else "rgba"), route
    guard.reset()
    dev_sets = [[(guard.dev((np.ascontiguousarray(img[..., :3]) if rgb else img).reshape(-1), "src", pitch=img.shape[1] * (12 if rgb else 16), label="job %d layer %d" % (j, i)),
                  img.shape[1], img.shape[0], mat) for i, (img, mat) in enumerate(s)] for j, s in enumerate(sets)]
    dsts = [guarded_outputs(outs, w, h, "job %d " % j) for j in range(2)]
    with capi.trace() as t:
        tails.compose_up_write_multi(dev_sets, [o for _, o in dsts], w, h, rgb=rgb)
    tails.wait()
    torch.cuda.synchronize()
    assert t.route == route, t.route
    n_src, n_dst = guard.check()
    assert n_src == 4 and n_dst == 2 * sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
    for j, (dst, _) in enumerate(dsts):
        same_as_plain(dst, plain[j], "job %d" % j)
