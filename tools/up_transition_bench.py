#!/usr/bin/env python3
"""Frames of a transition on a channel of enlarged (or own-size) packed fields: ONE ph_compose_up_transition_multi call against what makes
the same frames without it - every packed image of the frame unpacked in place (ph_image_unpack_rgb, one launch each) and
ph_chan_compose_multi with PH_SRC_RGBA_F32 sources, one call per job - in one process, the two sides alternating on warmed shapes, timed
with device events.  Shapes: four packed-RGB 1080p fields on a 1080p channel (the identity fill, a frame write) with one layer in a
dissolve and one in a wipe, for SDI, for SDI + the screen, and for both fields of a tick (two jobs, two mixes); BASELINE config 3
(4 x 1080p -> 2160p) with one layer dissolving.
  python tools/up_transition_bench.py [reps=200] [rounds=7] [out=profiles/up_transition_bench.jsonl] [only=<shape name>]
One JSON line per shape: the median of the rounds for both sides and the old side's spread (max - min over its rounds)."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "up_transition_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    wr_cm = {"v210": dev(capi.rgb2ycbcr_matrix("709")), "bgra8": None}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of image sets: no image is read from the cache the launch before left it in
    N = 4  # layers

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda")]
        return [torch.empty(w * h, dtype=torch.int32, device="cuda")]

    unpack_fn = capi.lib().ph_image_unpack_rgb

    def unpack_job(images, sw, sh):
        """ph_image_unpack_rgb on every image, the C calls alone (the images' contents are noise either way: only the time counts)"""
        args = [(ctx.h, capi.QUEUE_PROCESS, ctypes.c_void_p(t.data_ptr()), sw, sh) for t in images]

        def job(_keep=images):
            for a in args:
                capi.check(unpack_fn(*a), ctx.h)
        return job

    # (name, source size, frame size, jobs, outputs, {layer: kind})
    SRC = (1920, 1080)
    both = {1: "dissolve", 2: "wipe"}
    shapes = [("f3 dissolve+wipe v210", SRC, SRC, 1, ["v210"], both), ("f3 dissolve+wipe v210+bgra8", SRC, SRC, 1, ["v210", "bgra8"], both),
              ("f3 pair dissolve+wipe v210", SRC, SRC, 2, ["v210"], both), ("config3 dissolve v210", SRC, (3840, 2160), 1, ["v210"], {1: "dissolve"})]
    lines = []
    for name, (sw, sh), (w, h), jobs, outs, kinds in shapes:
        if only and only != name:
            continue
        mat = capi.transform_matrix(w, h)
        partners = [(l, key) for l, kind in sorted(kinds.items()) for key in (("incoming", "mask") if kind == "wipe" else ("incoming",))]
        images = N + len(partners)  # per job: the layers' fields, then the partners
        # per ring slot and job: the packed images the compositor reads, and buffers of the RGBA size that today's route unpacks in place
        packed = [[[torch.rand(sw * sh * 3, device="cuda") for _ in range(images)] for _ in range(jobs)] for _ in range(R)]
        rgba = [[[torch.rand(sw * sh * 4, device="cuda") for _ in range(images)] for _ in range(jobs)] for _ in range(R)]
        dst = [[frame(fmt, w, h) for fmt in outs] for _ in range(jobs)]
        torch.cuda.synchronize()
        outputs = [[dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst[j])] for j in range(jobs)]

        def layers(pool, j, source):
            """job j's layers from a pool of images; the two fields of a tick have two mixes"""
            ls = [dict(src=source(t), transition=kinds.get(l, "cut"), mix=0.4 + 0.02 * j) for l, t in enumerate(pool[:N])]
            for (l, key), t in zip(partners, pool[N:]):
                ls[l][key] = source(t)
            return ls
        new = [ctx.compose_up_transition_multi([layers(packed[s][j], j, lambda t: (t, sw, sh, mat)) for j in range(jobs)], outputs, w, h, rgb=True, prepare_only=True) for s in range(R)]

        def old_route(s):
            seq = []
            for j in range(jobs):
                seq.append(unpack_job(rgba[s][j], sw, sh))
                seq.append(ctx.chan_compose_multi(layers(rgba[s][j], j, lambda t: (t, sw, sh, mat, "rgba")), outputs[j], w, h, *rd, prepare_only=True))
            return seq
        old = [old_route(s) for s in range(R)]
        routes = {}
        with capi.trace(dry_run=True) as t:
            new[0]()
        routes["new"] = t.route
        with capi.trace(dry_run=True) as t:
            for job in old[0]:
                job()
        routes["old"] = t.route

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                fn(i % R)
            e1.record(stream)
            ctx.wait()
            return 1e3 * e0.elapsed_time(e1) / reps
        sides = {"new": lambda i: new[i](), "old": lambda i: [job() for job in old[i]]}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # until every shape is warm and the clocks have settled
            for fn in sides.values():
                for i in range(R):
                    fn(i)
            ctx.wait()
        us = {k: [] for k in sides}
        for _ in range(rounds):  # the sides alternate inside a round
            for k, fn in sides.items():
                us[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = max(us["old"]) - min(us["old"])
        line = {"bench": "up_transition", "shape": name, "source": [sw, sh], "width": w, "height": h, "layers": N, "transitions": {str(l): k for l, k in kinds.items()},
                "images": images, "jobs": jobs, "outputs": outs, "reps": reps, "rounds": rounds, "routes": routes, "new_us": round(med["new"], 2), "old_us": round(med["old"], 2),
                "old_spread_us": round(spread, 2), "new_spread_us": round(max(us["new"]) - min(us["new"]), 2), "saved_us": round(med["old"] - med["new"], 2),
                "new_wins_beyond_spread": bool(med["old"] - med["new"] > spread), "equal_within_spread": bool(abs(med["old"] - med["new"]) <= spread),
                "rounds_new_us": [round(v, 2) for v in us["new"]], "rounds_old_us": [round(v, 2) for v in us["old"]]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del packed, rgba, dst, new, old
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
