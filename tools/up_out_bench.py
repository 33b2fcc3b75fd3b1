#!/usr/bin/env python3
"""Frames of enlarged (or own-size) images for a channel's consumers: ONE ph_compose_up_write_multi call against what makes the same
frames without it - ph_compose_up_write_v210 for the SDI frame, and for every other consumer the fields unpacked in place
(ph_image_unpack_rgb, once per tick) and ph_chan_compose - in one process, the two sides alternating on warmed shapes, timed with
device events.  Shapes: f3 (four packed-RGB 1080p fields under the identity fill, a frame write) for one consumer that is not SDI, for
SDI + the screen, SDI + an encoder + the screen, both fields of a tick; BASELINE config 3 (4 x 1080p -> 2160p) for SDI + the screen;
and v210 alone through the new entry, which must be today's kernel.
  python tools/up_out_bench.py [reps=200] [rounds=7] [out=profiles/up_out_bench.jsonl] [only=<shape name> or "" : for a profiler run] [step=126]
One JSON line per shape: the median of the rounds for both sides and the separate side's spread (max - min over the rounds).
step=126: the A/B of the wave step's width - the library is told (PH_UP_OUT_STEP=126, read once when the first launch is made) to keep
126-column steps in launches without a v210 output too, where it takes 128; run it as a second process and write it beside the first
record (out=profiles/up_out_bench_step126.jsonl): the same separate side in both files says how far two processes may be compared."""
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
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "up_out_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    step = int(sys.argv[5].split("=")[-1]) if len(sys.argv) > 5 else 128
    if step == 126:
        os.environ["PH_UP_OUT_STEP"] = "126"  # (before the library is loaded)
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE[f])) for f in ("yuv422p8", "yuv420p", "rgba8", "bgra8")}
    wr_cm["v210"] = dev(capi.rgb2ycbcr_matrix("709"))
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of image sets: no image is read from the cache the launch before left it in
    N = 4  # layers

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda")]
        if fmt == "yuv422p8":
            return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in (w * h, w * h // 2, w * h // 2)]
        if fmt == "yuv420p":
            return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in (w * h, w * h // 4, w * h // 4)]
        return [torch.empty(w * h, dtype=torch.int32, device="cuda")]

    unpack_fn = capi.lib().ph_image_unpack_rgb

    def unpack_job(images, sw, sh):
        """ph_image_unpack_rgb on every image, the C calls alone (the images' contents are noise either way: only the time counts)"""
        args = [(ctx.h, capi.QUEUE_PROCESS, ctypes.c_void_p(t.data_ptr()), sw, sh) for t in images]

        def job(_keep=images):
            for a in args:
                capi.check(unpack_fn(*a), ctx.h)
        return job

    # (name, source size, frame size, jobs, outputs)
    SRC = (1920, 1080)
    shapes = [("f3 rgba8", SRC, SRC, 1, ["rgba8"]), ("f3 yuv422p8", SRC, SRC, 1, ["yuv422p8"]), ("f3 yuv420p", SRC, SRC, 1, ["yuv420p"]),
              ("f3 v210+bgra8", SRC, SRC, 1, ["v210", "bgra8"]), ("f3 v210+yuv422p8+rgba8", SRC, SRC, 1, ["v210", "yuv422p8", "rgba8"]),
              ("config3 v210+bgra8", SRC, (3840, 2160), 1, ["v210", "bgra8"]), ("f3 pair v210+bgra8", SRC, SRC, 2, ["v210", "bgra8"]),
              ("f3 v210 alone", SRC, SRC, 1, ["v210"])]
    lines = []
    for name, (sw, sh), (w, h), jobs, outs in shapes:
        if only and only != name:
            continue
        mat = capi.transform_matrix(w, h)
        # per ring slot and job: the packed fields the compositor reads, and buffers of the RGBA size that today's route unpacks in place
        packed = [[[torch.rand(sw * sh * 3, device="cuda") for _ in range(N)] for _ in range(jobs)] for _ in range(R)]
        rgba = [[[torch.rand(sw * sh * 4, device="cuda") for _ in range(N)] for _ in range(jobs)] for _ in range(R)]
        dst = [[frame(fmt, w, h) for fmt in outs] for _ in range(jobs)]
        torch.cuda.synchronize()
        outputs = [[dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst[j])] for j in range(jobs)]
        up_layers = lambda s, j: [(t, sw, sh, mat) for t in packed[s][j]]
        multi = [ctx.compose_up_write_multi([up_layers(s, j) for j in range(jobs)], outputs, w, h, rgb=True, prepare_only=True) for s in range(R)]

        def separate(s):
            seq = []
            others = [k for k, fmt in enumerate(outs) if fmt != "v210"]
            if "v210" in outs:
                k = outs.index("v210")
                if jobs == 2:
                    seq.append(ctx.compose_up_write_v210_pair(up_layers(s, 0), up_layers(s, 1), dst[0][k][0], dst[1][k][0], w, h, 0, wr_cm["v210"], wr_lut, rgb=True, prepare_only=True))
                else:
                    seq.append(ctx.compose_up_write_v210(up_layers(s, 0), dst[0][k][0], w, h, 0, wr_cm["v210"], wr_lut, rgb=True, prepare_only=True))
            for j in range(jobs):
                if others:
                    seq.append(unpack_job(rgba[s][j], sw, sh))
                for k in others:
                    ls = [dict(src=(t, sw, sh, mat, "rgba")) for t in rgba[s][j]]
                    seq.append(ctx.chan_compose_v210(ls, dst[j][k], w, h, 0, *rd, wr_cm[outs[k]], wr_lut, prepare_only=True, out_fmt=outs[k]))
            return seq
        alone = [separate(s) for s in range(R)]
        routes = {}
        with capi.trace(dry_run=True) as t:
            multi[0]()
        routes["multi"] = t.route
        with capi.trace(dry_run=True) as t:
            for job in alone[0]:
                job()
        routes["separate"] = t.route

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                fn(i % R)
            e1.record(stream)
            ctx.wait()
            return 1e3 * e0.elapsed_time(e1) / reps
        sides = {"multi": lambda i: multi[i](), "separate": lambda i: [job() for job in alone[i]]}
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
        spread = max(us["separate"]) - min(us["separate"])
        line = {"bench": "up_out", "shape": name, "step_without_v210": step, "source": [sw, sh], "width": w, "height": h, "layers": N, "jobs": jobs, "outputs": outs, "reps": reps, "rounds": rounds,
                "routes": routes, "multi_us": round(med["multi"], 2), "separate_us": round(med["separate"], 2), "separate_spread_us": round(spread, 2),
                "multi_spread_us": round(max(us["multi"]) - min(us["multi"]), 2), "saved_us": round(med["separate"] - med["multi"], 2),
                "multi_wins_beyond_spread": bool(med["separate"] - med["multi"] > spread), "equal_within_spread": bool(abs(med["separate"] - med["multi"]) <= spread),
                "rounds_multi_us": [round(v, 2) for v in us["multi"]], "rounds_separate_us": [round(v, 2) for v in us["separate"]]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del packed, rgba, dst, multi, alone
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
