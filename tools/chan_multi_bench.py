#!/usr/bin/env python3
"""Several consumers' frames of one channel: ONE ph_chan_compose_multi call against the separate calls that make the same frames
(one ph_chan_compose per consumer; the headline's v210 frame by ph_fused_v210_combine) - in one process, the two alternating on warmed
shapes, timed with device events.  Shapes: BASELINE config 2's frame (1080p, four v210 layers, insets, a wipe) for SDI + the screen,
SDI + an encoder, an SDI field + the screen's frame; the headline's shape (four plain 2160p reads) for SDI + the screen; a 1080p
yuv420p clip under the default fill for SDI + an encoder.
  python tools/chan_multi_bench.py [reps=200] [rounds=7] [out=profiles/chan_multi_bench.jsonl] [only=<shape name>: for a profiler run]
One JSON line per shape: the median of the rounds for both sides, the separate side's spread (max - min over the rounds), the first
output alone, and from those the cost of each added output."""
import json
import os
import statistics
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "chan_multi_bench.jsonl")
    only = sys.argv[4] if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    wr_cm = {"v210": dev(capi.rgb2ycbcr_matrix("709")), "yuv422p8": dev(capi.rgb2ycbcr_matrix("709", 8, 16, 235, 224)), "rgba8": None, "bgra8": None}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of source sets: no frame is read from the cache the launch before left it in

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda")]
        if fmt == "yuv422p8":
            return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in (w * h, w * h // 2, w * h // 2)]
        return [torch.empty(w * h, dtype=torch.int32, device="cuda")]

    def v210_sets(w, h, n):
        words = capi.v210_pitch_bytes(w) * h // 4
        return [[torch.randint(0, 2 ** 30, (words,), dtype=torch.int32, device="cuda") for _ in range(n)] for _ in range(R)]

    def config2(w, h):
        mask = torch.zeros(h, w, 4, device="cuda")
        mask[..., 0] = torch.linspace(0, 1, w, device="cuda")[None, :]
        mask = mask.reshape(-1).contiguous()
        mats = [capi.transform_matrix(w, h)] + [capi.transform_matrix(w, h, scale_x=0.5, scale_y=0.5, offset_x=ox, offset_y=oy) for ox, oy in ((-0.25, -0.25), (0.25, -0.25), (0.25, 0.25))]
        sets = []
        for s in v210_sets(w, h, 5):
            ls = [dict(src=(s[l], w, h, mats[l])) for l in range(4)]
            ls[3].update(transition="wipe", incoming=(s[4], w, h, None), mask=(mask, w, h, None, "rgba"))
            sets.append(ls)
        return sets

    def headline(w, h):
        return [[dict(src=(x, w, h, None)) for x in s] for s in v210_sets(w, h, 4)]

    def clip(w, h):
        plane = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
        own = dev(capi.ycbcr2rgb_matrix("709", 8, 16, 235, 224))
        return [[dict(src=((plane(w * h), plane(w * h // 4), plane(w * h // 4)), w, h, capi.transform_matrix(w, h), "yuv420p", own))] for _ in range(R)]

    shapes = [("config2 v210+bgra8", 1920, 1080, config2, [("v210", 0), ("bgra8", 0)], None),
              ("config2 v210+yuv422p8", 1920, 1080, config2, [("v210", 0), ("yuv422p8", 0)], None),
              ("config2 v210 field+rgba8 frame", 1920, 1080, config2, [("v210", 1), ("rgba8", 0)], None),
              ("headline 2160p v210+bgra8", 3840, 2160, headline, [("v210", 0), ("bgra8", 0)], "fused"),
              ("yuv420p clip 1080p v210+yuv422p8", 1920, 1080, clip, [("v210", 0), ("yuv422p8", 0)], None)]
    made = {}
    lines = []
    for name, w, h, make, outs, first_by in shapes:
        if only and only != name:
            continue
        if (make, w, h) not in made:
            made = {(make, w, h): make(w, h)}  # (one shape's sources at a time)
        sets = made[(make, w, h)]
        dst = [frame(fmt, w, h) for fmt, _ in outs]
        torch.cuda.synchronize()
        outputs = [dict(fmt=fmt, planes=d, interlace=il, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for (fmt, il), d in zip(outs, dst)]
        multi = [ctx.chan_compose_multi(ls, outputs, w, h, *rd, prepare_only=True) for ls in sets]

        def one(ls, k):
            fmt, il = outs[k]
            if k == 0 and first_by == "fused":  # the headline's own kernel makes its v210 frame
                return ctx.fused_v210_combine([L["src"][0] for L in ls], dst[0][0], w, h, *rd, wr_cm["v210"], wr_lut, prepare_only=True)
            return ctx.chan_compose_v210(ls, dst[k][0] if fmt == "v210" else dst[k], w, h, il, *rd, wr_cm[fmt], wr_lut, prepare_only=True, out_fmt=fmt)
        alone = [[one(ls, k) for k in range(len(outs))] for ls in sets]
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
        sides = {"multi": lambda i: multi[i](), "separate": lambda i: [job() for job in alone[i]], "first_alone": lambda i: alone[i][0]()}
        import time
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
        line = {"bench": "chan_multi", "shape": name, "width": w, "height": h, "outputs": ["%s il %d" % o for o in outs], "reps": reps, "rounds": rounds, "routes": routes,
                "multi_us": round(med["multi"], 2), "separate_us": round(med["separate"], 2), "first_output_alone_us": round(med["first_alone"], 2),
                "separate_spread_us": round(spread, 2), "multi_spread_us": round(max(us["multi"]) - min(us["multi"]), 2),
                "saved_us": round(med["separate"] - med["multi"], 2), "multi_wins_beyond_spread": bool(med["separate"] - med["multi"] > spread),
                "added_output_us_multi": round((med["multi"] - med["first_alone"]) / (len(outs) - 1), 2),
                "added_output_us_separate": round((med["separate"] - med["first_alone"]) / (len(outs) - 1), 2),
                "rounds_multi_us": [round(v, 2) for v in us["multi"]], "rounds_separate_us": [round(v, 2) for v in us["separate"]]}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
