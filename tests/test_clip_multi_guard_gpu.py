"""GPU tests (-m gpu): ph_clip_compose_multi's one-launch route and its two-stage route with every source plane and every output plane
between guard bands (tests/guard.py).  A store outside a plane damages a guard and guard.check() names it; a load outside a source plane
brings a value (0xFF codes) that changes the frame, which is compared with the one made from plain buffers."""
import numpy as np
import pytest

import frames
import guard
import packfmt
from test_chan_gpu import Src, colour, m
from test_chan_multi_gpu import out, poisoned, writer
from test_clip_multi_gpu import check_clip, two_stage

pytestmark = pytest.mark.gpu

CASES = [("yuv420p", 100, 24, 384, 34, dict(), ["nv12", "v210", "rgba8"]),
         # (the taps of the frame's rim leave the clip on every side: transform.ts:53 samples half a texel off the pixel centres)
         ("p010", 52, 8, 128, 10, dict(), ["yuv422p8", "bgra8", "yuv420p"])]


def guarded_source(src):
    from phaneron_amd import capi
    f = packfmt.get(src.fmt)
    planes = tuple(guard.dev(np.ascontiguousarray(p).reshape(-1), "src", pitch=np.ascontiguousarray(p).nbytes // src.h, label="%s plane %d" % (src.fmt, i)) for i, p in enumerate(src.data))
    own = guard.dev(capi.ycbcr2rgb_matrix(src.spec, *f.code_range), "src", label="the source's own matrix") if src.own_matrix() else None
    return (planes, src.w, src.h, src.matrix, src.fmt, own)


@pytest.mark.parametrize("option", [1, 2])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_routes_between_guards(case, option):
    import torch
    import hip_harness as hh
    fmt, sw, sh, w, h, kw, fmts = CASES[case]
    src = Src.random(fmt, sw, sh, 2300 + case, m(w, h, **kw))
    outs = [out(f, il) for f, il in zip(fmts, (0, 3, 0))]
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    k.set_option("chan_enlarged", option)
    try:
        route, plain = check_clip([dict(src=src)], w, h, outs, "%s %dx%d on %dx%d, plain buffers" % (fmt, sw, sh, w, h), separate=False)
        guard.reset()
        recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
        dst = [[guard.dev(p, "dst", pitch=p.nbytes // h, label="%s plane %d" % (o["fmt"], i)) for i, p in enumerate(poisoned(o["fmt"], w, h))] for o in outs]
        outputs = [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]
        k.clip_compose_multi([dict(src=guarded_source(src), transition="cut", mix=0.0)], outputs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        n_src, n_dst = guard.check()
        assert n_src == len(src.data) + int(src.own_matrix()) and n_dst == sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
        for i, d in enumerate(dst):
            for pl, p in enumerate(d):
                assert np.array_equal(hh.host(p, np.uint8), plain[i][pl]), "output %d plane %d differs from the frame made from plain buffers" % (i, pl)
    finally:
        k.set_option("chan_enlarged", 1)
        guard.reset()
    assert route == "clip_up_multi<rgb>x3" if option == 1 else two_stage(route, 3), route
