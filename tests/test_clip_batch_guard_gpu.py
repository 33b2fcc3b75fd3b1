"""GPU tests (-m gpu): a 3-job, 3-output launch of ph_clip_compose_batch_out with every source plane and every output plane between
guard bands (tests/guard.py).  A store outside a plane damages a guard and guard.check() names it; a load outside a source plane brings a
value (0xFF codes) that changes the frame, which is compared with the one ph_clip_compose_multi makes from plain buffers."""
import numpy as np
import pytest

import frames
import guard
from test_chan_gpu import Src, colour, m
from test_chan_multi_gpu import out, poisoned, writer
from test_clip_multi_gpu import check_clip
from test_clip_multi_guard_gpu import guarded_source

pytestmark = pytest.mark.gpu

CASES = [(("yuv420p", "nv12", "yuv422p10"), 100, 24, 384, 34, ["nv12", "v210", "rgba8"]),
         # (the taps of the frame's rim leave the clip on every side: transform.ts:53 samples half a texel off the pixel centres)
         (("p010", "yuv420p10", "yuv422p8"), 52, 8, 128, 10, ["yuv422p8", "bgra8", "yuv420p"])]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_a_shared_launch_between_guards(case):
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    fmts, sw, sh, w, h, ofmts = CASES[case]
    srcs = [Src.random(f, sw, sh, 2400 + 10 * case + j, m(w, h)) for j, f in enumerate(fmts)]
    outs = [out(f, il) for f, il in zip(ofmts, (0, 3, 0))]
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    plain = [check_clip([dict(src=s)], w, h, outs, "job %d from plain buffers" % j, separate=False)[1] for j, s in enumerate(srcs)]
    guard.reset()
    try:
        recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
        jobs, dsts = [], []
        for j, s in enumerate(srcs):
            dst = [[guard.dev(p, "dst", pitch=p.nbytes // h, label="job %d %s plane %d" % (j, o["fmt"], i)) for i, p in enumerate(poisoned(o["fmt"], w, h))] for o in outs]
            outputs = [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]
            jobs.append(([dict(src=guarded_source(s), transition="cut", mix=0.0)], outputs))
            dsts.append(dst)
        with capi.trace() as t:
            k.clip_compose_batch_out(jobs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        assert t.route == "clip_up_multi<rgb>x3j3", t.route
        n_src, n_dst = guard.check()
        assert n_src == sum(len(s.data) + int(s.own_matrix()) for s in srcs) and n_dst == 3 * sum(len(frames.pack_plane_bytes(f, w, h)) for f in ofmts)
        for j, dst in enumerate(dsts):
            for i, d in enumerate(dst):
                for pl, p in enumerate(d):
                    assert np.array_equal(hh.host(p, np.uint8), plain[j][i][pl]), "job %d output %d plane %d differs from the frame made from plain buffers" % (j, i, pl)
    finally:
        guard.reset()
