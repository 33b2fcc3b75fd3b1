#!/usr/bin/env python3
"""Several channels' plain-layer composites, each for the same consumers: ONE ph_fused_v210_combine_multi_batch call against the parent's
way to make the same frames - `jobs` separate ph_fused_v210_combine_multi calls - in one process, the sides alternating on warmed
shapes, timed with device events.  The jobs' layers cycle over a ring of frame sets larger than the 256 MiB Infinity Cache, as
bench.py's headline does.
  python tools/fused_multi_batch_bench.py [reps=1000] [rounds=7] [out=profiles/fused_multi_batch_bench.jsonl] [only=<shape name>]
One JSON line per shape: the median of the rounds for each side (microseconds per launch of the shared side = per `jobs` frames) and
each side's spread (max - min over the rounds).  The baseline is the separate-calls side of this very run; the shared call counts as
faster only if it wins by more than that side's spread."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

CACHE_BYTES = 256 << 20
SHAPES = [(4, "1080p", ["yuv422p8"]), (4, "1080p", ["v210", "bgra8"]), (8, "1080p", ["nv12"]), (2, "2160p", ["yuv422p8"]), (2, "1080p", ["v210", "yuv422p8", "rgba8"])]
SIZES = {"2160p": (3840, 2160), "1080p": (1920, 1080)}


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "fused_multi_batch_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rspec, wspec, n = "709", "2020", 4
    rd_lut_h, wr_lut_h = capi.gamma2linear_lut(rspec), capi.linear2gamma_lut(wspec)
    rd = (dev(capi.ycbcr2rgb_matrix(rspec)), dev(rd_lut_h), dev(np.concatenate([capi.rgb2rgb_matrix(rspec, wspec), np.zeros(3, np.float32)])))
    wr_lut = dev(wr_lut_h)
    fmts = ("v210", "yuv422p8", "nv12", "rgba8", "bgra8")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix(wspec, *capi.FORMAT_RANGE[f])) for f in fmts}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], rd_lut_h)
    ctx.register_lut(wr_lut, wr_lut_h)

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h, dtype=torch.uint8, device="cuda")]
        return [torch.empty(b, dtype=torch.uint8, device="cuda") for b in capi.pack_plane_bytes(fmt, w, h)]

    lines = []
    for jobs, size, outs in SHAPES:
        w, h = SIZES[size]
        name = "%d x %s %s" % (jobs, size, "+".join(outs))
        if only and only != name:
            continue
        frame_bytes = capi.v210_pitch_bytes(w) * h
        ring = CACHE_BYTES // (jobs * n * frame_bytes) + 2
        gen = torch.Generator(device="cuda").manual_seed(5)
        # a ring of ticks: every tick has the layers of all its jobs
        sets = [[[torch.randint(0, 2 ** 31 - 1, (frame_bytes // 4,), dtype=torch.int32, device="cuda", generator=gen) & 0x3FFFFFFF for _ in range(n)] for _ in range(jobs)]
                for _ in range(ring)]
        dst = [[frame(fmt, w, h) for fmt in outs] for _ in range(jobs)]
        torch.cuda.synchronize()
        outputs = [[dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst[j])] for j in range(jobs)]
        shared = [ctx.fused_v210_combine_multi_batch(tick, outputs, w, h, *rd, prepare_only=True) for tick in sets]

        def apart(tick):
            calls = [ctx.fused_v210_combine_multi(tick[j], outputs[j], w, h, *rd, prepare_only=True) for j in range(jobs)]

            def job():
                for c in calls:
                    c()
            return job
        separate = [apart(tick) for tick in sets]
        sides = {"shared": shared, "separate": separate}
        routes = {}
        for k, side in sides.items():
            with capi.trace(dry_run=True) as t:
                side[0]()
            routes[k] = t.route

        def timed(side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                side[i % ring]()
            e1.record(stream)
            ctx.wait()
            return 1e3 * e0.elapsed_time(e1) / reps
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # until every side is warm and the clocks have settled
            for side in sides.values():
                for job in side:
                    job()
            ctx.wait()
        us = {k: [] for k in sides}
        for _ in range(rounds):  # the sides alternate inside a round
            for k, side in sides.items():
                us[k].append(timed(side))
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        saved = med["separate"] - med["shared"]
        line = {"bench": "fused_multi_batch", "shape": name, "jobs": jobs, "width": w, "height": h, "layers": n, "frame_sets": ring, "outputs": outs, "reps": reps, "rounds": rounds,
                "routes": routes, "shared_us": round(med["shared"], 2), "separate_us": round(med["separate"], 2), "shared_spread_us": round(spread["shared"], 2),
                "separate_spread_us": round(spread["separate"], 2), "shared_us_per_frame": round(med["shared"] / jobs, 2), "separate_us_per_frame": round(med["separate"] / jobs, 2),
                "saved_us": round(saved, 2), "saved_us_per_frame": round(saved / jobs, 2), "shared_wins_beyond_spread": bool(saved > spread["separate"]),
                "shared_loses_beyond_spread": bool(-saved > spread["separate"]), "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dst, shared, separate, sets
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
