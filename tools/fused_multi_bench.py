#!/usr/bin/env python3
"""The plain-layer composite for several consumers: ONE ph_fused_v210_combine_multi call against the two ways the parent has to make
the same frames - (a) one ph_chan_compose_multi / ph_chan_compose call on the layers taken 1:1, (b) ph_fused_v210_combine for the
v210 frame plus a ph_chan_compose per other output (without a v210 output, (b) is a ph_chan_compose per output) - in one process,
the sides alternating on warmed shapes, timed with device events.  The layers cycle over a ring of frame sets larger than the
256 MiB Infinity Cache, as bench.py's headline does.
  python tools/fused_multi_bench.py [reps=1000] [rounds=7] [out=profiles/fused_multi_bench.jsonl] [only=<shape name>]
One JSON line per shape: the median of the rounds for every side and each side's spread (max - min over the rounds).  The baseline
is the better of (a) and (b) in this very run; the new call counts as faster only if it wins by more than that baseline's spread.
Kernels alone: run the tool under `rocprofv3 --kernel-trace --stats` with reps=50 rounds=1 and a throw-away out file."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

CACHE_BYTES = 256 << 20


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "fused_multi_bench.jsonl")
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

    sizes = [("2160p", 3840, 2160), ("1080p", 1920, 1080)]
    mixes = [["yuv422p8"], ["nv12"], ["v210", "bgra8"], ["v210", "yuv422p8", "rgba8"]]
    lines = []
    for size, w, h in sizes:
        frame_bytes = capi.v210_pitch_bytes(w) * h
        ring = CACHE_BYTES // (n * frame_bytes) + 2
        gen = torch.Generator(device="cuda").manual_seed(5)
        sets = [[torch.randint(0, 2 ** 31 - 1, (frame_bytes // 4,), dtype=torch.int32, device="cuda", generator=gen) & 0x3FFFFFFF for _ in range(n)] for _ in range(ring)]
        for outs in mixes:
            name = "%s %s" % (size, "+".join(outs))
            if only and only != name:
                continue
            dst = [frame(fmt, w, h) for fmt in outs]
            torch.cuda.synchronize()
            outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
            chan = [[dict(src=(t, w, h, None), transition="cut", mix=0.0) for t in layers] for layers in sets]
            new = [ctx.fused_v210_combine_multi(layers, outputs, w, h, *rd, prepare_only=True) for layers in sets]
            one_call = [ctx.chan_compose_multi(cl, outputs, w, h, *rd, prepare_only=True) for cl in chan]

            def per_output(layers, cl):
                jobs = []
                for fmt, d in zip(outs, dst):
                    if fmt == "v210":
                        jobs.append(ctx.fused_v210_combine(layers, d[0], w, h, *rd, wr_cm[fmt], wr_lut, prepare_only=True))
                    else:
                        jobs.append(ctx.chan_compose_v210(cl, d, w, h, 0, *rd, wr_cm[fmt], wr_lut, prepare_only=True, out_fmt=fmt))

                def job():
                    for j in jobs:
                        j()
                return job
            apart = [per_output(layers, cl) for layers, cl in zip(sets, chan)]
            sides = {"new": new, "one_chan_call": one_call, "headline_plus_chan_calls": apart}
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
            base = min(("one_chan_call", "headline_plus_chan_calls"), key=lambda k: med[k])
            line = {"bench": "fused_multi", "shape": name, "width": w, "height": h, "layers": n, "frame_sets": ring, "outputs": outs, "reps": reps, "rounds": rounds, "routes": routes,
                    "new_us": round(med["new"], 2), "one_chan_call_us": round(med["one_chan_call"], 2), "headline_plus_chan_calls_us": round(med["headline_plus_chan_calls"], 2),
                    "baseline": base, "baseline_us": round(med[base], 2), "baseline_spread_us": round(spread[base], 2), "new_spread_us": round(spread["new"], 2),
                    "saved_us": round(med[base] - med["new"], 2), "new_wins_beyond_spread": bool(med[base] - med["new"] > spread[base]),
                    "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del dst, new, one_call, apart, chan
        del sets
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
