"""GPU tests (-m gpu): ph_clip_compose_route_multi's one-launch route and its two-stage route with every source plane, image_out and
every output plane between guard bands (tests/guard.py).  A store outside a plane or the image damages a guard and guard.check() names
it; a load outside a source plane brings a value (0xFF codes) that changes the frame and the image, which are compared with those made
from plain buffers.  The sizes put the frame's edges inside tiles and wave steps: 384 x 34 is three 126-column steps and a fourth of 6
columns, 128 x 10 one step of 2 columns past the first, 130 x 7 an odd height whose last row pair is a single row."""
import numpy as np
import pytest

import frames
import guard
from test_chan_gpu import Src, colour, m
from test_chan_multi_gpu import out, poisoned, writer
from test_clip_multi_guard_gpu import guarded_source
from test_clip_route_gpu import check_route, two_stage
from test_fused_route_gpu import poison_image

pytestmark = pytest.mark.gpu

CASES = [("yuv420p", 100, 24, 384, 34, dict(), ["nv12", "v210", "rgba8"]),
         # (the taps of the frame's rim leave the clip on every side: transform.ts:53 samples half a texel off the pixel centres)
         ("p010", 52, 8, 128, 10, dict(), ["yuv422p8", "bgra8", "yuv420p"]),
         ("bgra8", 60, 4, 130, 7, dict(scale_x=0.9, offset_x=0.2), ["rgba8", "bgra8"]),
         ("yuv422p10", 128, 10, 128, 10, dict(), [])]  # the default fill, the image alone


def guarded(src):
    g = guarded_source(src)
    return (g[0][0],) + g[1:5] if src.fmt in ("rgba8", "bgra8") else g  # (packed 8-bit pixels: one tensor, not a tuple of planes)


@pytest.mark.parametrize("option", [1, 2])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_routes_between_guards(case, option):
    import torch
    import hip_harness as hh
    fmt, sw, sh, w, h, kw, fmts = CASES[case]
    src = Src.random(fmt, sw, sh, 6800 + case, m(w, h, **kw))
    outs = [out(f, il) for f, il in zip(fmts, (0, 3, 0))]
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    k.set_option("chan_enlarged", option)
    try:
        route, plain, plain_image = check_route([dict(src=src)], w, h, outs, "%s %dx%d on %dx%d, plain buffers" % (fmt, sw, sh, w, h), sibling=False)
        guard.reset()
        recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
        dst = [[guard.dev(p, "dst", pitch=p.nbytes // h, label="%s plane %d" % (o["fmt"], i)) for i, p in enumerate(poisoned(o["fmt"], w, h))] for o in outs]
        outputs = [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]
        image_out = guard.dev(poison_image(w, h).reshape(-1), "dst", pitch=w * 16, label="image_out")
        k.clip_compose_route_multi([dict(src=guarded(src), transition="cut", mix=0.0)], image_out, outputs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        n_src, n_dst = guard.check()
        assert n_src == len(src.data) + int(src.own_matrix()) and n_dst == 1 + sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
        for i, d in enumerate(dst):
            for pl, p in enumerate(d):
                assert np.array_equal(hh.host(p, np.uint8), plain[i][pl]), "output %d plane %d differs from the frame made from plain buffers" % (i, pl)
        got = hh.host(image_out, np.float32).reshape(-1).view(np.uint32)
        assert np.array_equal(got, np.ascontiguousarray(plain_image).reshape(-1).view(np.uint32)), "image_out differs from the image made from plain buffers"
    finally:
        k.set_option("chan_enlarged", 1)
        guard.reset()
    inst = "rgba" if fmt in ("rgba8", "bgra8") else "rgb"
    assert route == "clip_up_route<%s>x%d" % (inst, len(fmts)) if option == 1 else two_stage(route, len(fmts), reads=1), route
