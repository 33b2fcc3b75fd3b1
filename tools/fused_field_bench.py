#!/usr/bin/env python3
"""An interlaced channel's frames through the plain-layer launches: the same ph_fused_v210_combine_multi / ph_fused_v210_combine_multi_batch
call with the context option "fused_fields" 0 (the whole frame composed, the field's quads stored - the parent's kernel, instruction for
instruction: profiles/fused_field_resources.txt) and 1 (only the field composed), and ph_chan_compose / ph_chan_compose_multi on the layers
taken 1:1 with the same outputs (the channel kernel composes the field only already; a batch is one such call per job).  One process, the
sides alternating inside every round on warmed shapes, timed with device events; the layers cycle over a ring of frame sets larger than
the 256 MiB Infinity Cache, as bench.py's headline does.  4 layers, every output field 1.
  python tools/fused_field_bench.py [reps=1000] [rounds=7] [out=profiles/fused_field_bench.jsonl] [only=<shape name>]
One JSON line per shape: every side's median of the rounds, per call and per frame, and its spread (max - min over the rounds).  The
baseline is option 0; option 1 wins or loses only by more than the baseline's spread.  No figure is a pass condition."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

CACHE_BYTES = 256 << 20
SIZES = {"1080p": (1920, 1080), "2160p": (3840, 2160)}
SHAPES = [(1, "1080p", ["v210"]), (1, "1080p", ["v210", "yuv422p8"]), (4, "1080p", ["v210"]), (4, "1080p", ["v210", "nv12"]), (1, "2160p", ["v210"])]
FIELD = 1


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "fused_field_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rspec, wspec, n = "709", "2020", 4
    rd_lut_h, wr_lut_h = capi.gamma2linear_lut(rspec), capi.linear2gamma_lut(wspec)
    rd = (dev(capi.ycbcr2rgb_matrix(rspec)), dev(rd_lut_h), dev(np.concatenate([capi.rgb2rgb_matrix(rspec, wspec), np.zeros(3, np.float32)])))
    wr_lut = dev(wr_lut_h)
    fmts = ("v210", "yuv422p8", "nv12")
    wr_cm = {f: dev(capi.rgb2ycbcr_matrix(wspec, *capi.FORMAT_RANGE[f])) for f in fmts}
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
        name = "%s%s %s field %d" % ("%d x " % jobs if jobs > 1 else "", size, "+".join(outs), FIELD)
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
        outputs = [[dict(fmt=fmt, planes=d, interlace=FIELD, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst[j])] for j in range(jobs)]
        if jobs > 1:
            fused = [ctx.fused_v210_combine_multi_batch(tick, outputs, w, h, *rd, prepare_only=True) for tick in sets]
        else:
            fused = [ctx.fused_v210_combine_multi(tick[0], outputs[0], w, h, *rd, prepare_only=True) for tick in sets]

        def chan_tick(tick):
            calls = [ctx.chan_compose_multi([dict(src=(t, w, h, None), transition="cut", mix=0.0) for t in tick[j]], outputs[j], w, h, *rd, prepare_only=True) for j in range(jobs)]

            def job():
                for c in calls:
                    c()
            return job
        # (side, the option's value while it runs, its jobs): the two fused sides are the same prepared calls - the option is read per call
        sides = [("frame", 0, fused), ("field", 1, fused), ("chan", 0, [chan_tick(tick) for tick in sets])]
        routes = {}
        for k, opt, side in sides:
            ctx.set_option("fused_fields", opt)
            with capi.trace(dry_run=True) as t:
                side[0]()
            routes[k] = t.route

        def timed(opt, side):
            ctx.set_option("fused_fields", opt)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                side[i % ring]()
            e1.record(stream)
            ctx.wait()
            return 1e3 * e0.elapsed_time(e1) / reps
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # until every side is warm and the clocks have settled
            for _, opt, side in sides:
                ctx.set_option("fused_fields", opt)
                for job in side:
                    job()
            ctx.wait()
        us = {k: [] for k, _, _ in sides}
        for _ in range(rounds):  # the sides alternate inside a round
            for k, opt, side in sides:
                us[k].append(timed(opt, side))
        ctx.set_option("fused_fields", 0)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        saved = med["frame"] - med["field"]
        line = {"bench": "fused_field", "shape": name, "width": w, "height": h, "layers": n, "jobs": jobs, "frame_sets": ring, "outputs": outs, "interlace": FIELD, "reps": reps,
                "rounds": rounds, "routes": routes}
        for k in ("frame", "field", "chan"):
            line["%s_us" % k] = round(med[k], 2)
            line["%s_us_per_frame" % k] = round(med[k] / jobs, 2)
            line["%s_spread_us" % k] = round(spread[k], 2)
        line.update({"baseline": "frame", "saved_us": round(saved, 2), "saved_percent": round(100.0 * saved / med["frame"], 1),
                     "wins_beyond_spread": bool(saved > spread["frame"]), "loses_beyond_spread": bool(-saved > spread["frame"]),
                     "field_beats_chan_beyond_spread": bool(med["chan"] - med["field"] > spread["chan"]),
                     "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dst, fused, sides, sets
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
