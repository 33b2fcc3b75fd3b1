"""GPU tests (-m gpu): ph_clip_compose_transition_multi's one-launch route and its two-stage route with every plane of every clip - src,
incoming, mask - and every output plane between guard bands (tests/guard.py).  A store outside a plane damages a guard and guard.check()
names it; a load outside a source plane brings a value (0xFF codes) that changes the frame, which is compared with the one made from
plain buffers.  The partners are smaller than the layer and placed differently: their rectangles are bounded by their own taps."""
import numpy as np
import pytest

import frames
import guard
from test_chan_gpu import Src, colour, m
from test_chan_multi_gpu import out, poisoned, writer
from test_clip_multi_guard_gpu import guarded_source
from test_clip_trans_gpu import check_trans, two_stage

pytestmark = pytest.mark.gpu

# (channel, kind, [(format, width, height, placement)]: src, incoming, mask; outputs)
CASES = [((384, 34), "wipe", [("yuv420p", 100, 24, dict()), ("nv12", 80, 20, dict(scale_x=0.9, scale_y=0.9, offset_x=0.1)), ("yuv422p10", 48, 12, dict(offset_y=-0.2))],
          ["nv12", "v210", "rgba8"]),
         # (the taps of the frame's rim leave the clips on every side: transform.ts:53 samples half a texel off the pixel centres)
         ((128, 10), "dissolve", [("p010", 52, 8, dict()), ("yuv422p8", 40, 6, dict(scale_x=0.8, offset_x=-0.3))], ["yuv422p8", "bgra8", "yuv420p"])]


@pytest.mark.parametrize("option", [1, 2])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_routes_between_guards(case, option):
    import torch
    import hip_harness as hh
    (w, h), kind, clips, fmts = CASES[case]
    images = [Src.random(fmt, sw, sh, 3300 + 4 * case + i, m(w, h, **kw)) for i, (fmt, sw, sh, kw) in enumerate(clips)]
    roles = ["src", "incoming", "mask"][:len(images)]
    layer = dict(zip(roles, images), transition=kind, mix=0.3)
    outs = [out(f, il) for f, il in zip(fmts, (0, 3, 0))]
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    k.set_option("chan_enlarged", option)
    try:
        route, plain = check_trans([layer], w, h, outs, "%s of %r on %dx%d, plain buffers" % (kind, clips, w, h), separate=False)
        guard.reset()
        recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
        dst = [[guard.dev(p, "dst", pitch=p.nbytes // h, label="%s plane %d" % (o["fmt"], i)) for i, p in enumerate(poisoned(o["fmt"], w, h))] for o in outs]
        outputs = [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]
        guarded = dict({role: guarded_source(s) for role, s in zip(roles, images)}, transition=kind, mix=0.3)
        k.clip_compose_transition_multi([guarded], outputs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        n_src, n_dst = guard.check()
        assert n_src == sum(len(s.data) + int(s.own_matrix()) for s in images) and n_dst == sum(len(frames.pack_plane_bytes(f, w, h)) for f in fmts)
        for i, d in enumerate(dst):
            for pl, p in enumerate(d):
                assert np.array_equal(hh.host(p, np.uint8), plain[i][pl]), "output %d plane %d differs from the frame made from plain buffers" % (i, pl)
    finally:
        k.set_option("chan_enlarged", 1)
        guard.reset()
    assert route == "clip_up_trans<rgb>x3" if option == 1 else two_stage(route, 3, reads=len(images)), route
