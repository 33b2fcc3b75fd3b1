#!/usr/bin/env python3
"""One f32 RGBA image packed for several consumers: ONE ph_pack_write_multi call against the separate ph_pack_write calls that make the
same frames, in one process, the two sides alternating on warmed shapes, timed with device events.  Every shape runs twice: cycling
over enough distinct images to exceed the 256 MiB Infinity Cache (what the shared read is worth when the image comes from HBM), and on
one image (when the cache may already serve the second and third read).
  python tools/pack_write_multi_bench.py [reps=100] [rounds=7] [out=profiles/pack_write_multi_bench.jsonl] [only=<shape name>]
One JSON line per shape and mode: the median of the rounds for both sides and the separate side's spread (max - min over the rounds).
A shape counts as faster only if it wins by more than that spread."""
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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pack_write_multi_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    spec = "2020"
    wr_lut = dev(capi.linear2gamma_lut(spec))
    fmts = ("v210", "p010", "yuv420p10", "yuv422p8", "nv12", "rgba8")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix(spec, *capi.FORMAT_RANGE[f])) for f in fmts}
    torch.cuda.synchronize()
    ctx.register_lut(wr_lut, capi.linear2gamma_lut(spec))

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h, dtype=torch.uint8, device="cuda")]
        return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in capi.pack_plane_bytes(fmt, w, h)]

    shapes = [("2160p v210+rgba8", 3840, 2160, ["v210", "rgba8"]), ("1080p v210+rgba8", 1920, 1080, ["v210", "rgba8"]),
              ("2160p v210+p010+rgba8", 3840, 2160, ["v210", "p010", "rgba8"]), ("1080p v210+p010+rgba8", 1920, 1080, ["v210", "p010", "rgba8"]),
              ("2160p v210+yuv422p8+rgba8", 3840, 2160, ["v210", "yuv422p8", "rgba8"]), ("2160p yuv420p10 alone", 3840, 2160, ["yuv420p10"]),
              ("720p nv12+rgba8", 1280, 720, ["nv12", "rgba8"])]
    lines = []
    for name, w, h, outs in shapes:
        if only and only != name:
            continue
        image_bytes = w * h * 16
        for mode in ("cycling", "one image"):
            ring = CACHE_BYTES // image_bytes + 2 if mode == "cycling" else 1
            images = [torch.rand(w * h * 4, device="cuda") for _ in range(ring)]
            dst = [frame(fmt, w, h) for fmt in outs]
            torch.cuda.synchronize()
            outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
            multi = [ctx.pack_write_multi(img, outputs, w, h, prepare_only=True) for img in images]
            fn = capi.lib().ph_pack_write

            def separate_job(img):
                import ctypes as C
                calls = []
                for fmt, d in zip(outs, dst):
                    arr = (C.c_void_p * 3)(*([p.data_ptr() for p in d] + [None] * (3 - len(d))))
                    calls.append((ctx.h, capi.QUEUE_PROCESS, capi.FORMATS[fmt], C.c_void_p(img.data_ptr()), arr, w, h, 0,
                                  None if wr_cm[fmt] is None else C.c_void_p(wr_cm[fmt].data_ptr()), C.c_void_p(wr_lut.data_ptr())))

                def job():
                    for a in calls:
                        capi.check(fn(*a), ctx.h)
                return job
            alone = [separate_job(img) for img in images]
            routes = {}
            with capi.trace(dry_run=True) as t:
                multi[0]()
            routes["multi"] = t.route
            with capi.trace(dry_run=True) as t:
                alone[0]()
            routes["separate"] = t.route

            def timed(side):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(reps):
                    side[i % ring]()
                e1.record(stream)
                ctx.wait()
                return 1e3 * e0.elapsed_time(e1) / reps
            sides = {"multi": multi, "separate": alone}
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:  # until every shape is warm and the clocks have settled
                for side in sides.values():
                    for job in side:
                        job()
                ctx.wait()
            us = {k: [] for k in sides}
            for _ in range(rounds):  # the sides alternate inside a round
                for k, side in sides.items():
                    us[k].append(timed(side))
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = max(us["separate"]) - min(us["separate"])
            moved = image_bytes + sum(sum(p.numel() for p in d) for d in dst)
            line = {"bench": "pack_write_multi", "shape": name, "mode": mode, "images": ring, "width": w, "height": h, "outputs": outs, "reps": reps, "rounds": rounds,
                    "routes": routes, "multi_us": round(med["multi"], 2), "separate_us": round(med["separate"], 2), "separate_spread_us": round(spread, 2),
                    "multi_spread_us": round(max(us["multi"]) - min(us["multi"]), 2), "saved_us": round(med["separate"] - med["multi"], 2),
                    "multi_wins_beyond_spread": bool(med["separate"] - med["multi"] > spread), "equal_within_spread": bool(abs(med["separate"] - med["multi"]) <= spread),
                    "multi_gb_s": round(moved / med["multi"] / 1e3, 1),
                    "rounds_multi_us": [round(v, 2) for v in us["multi"]], "rounds_separate_us": [round(v, 2) for v in us["separate"]]}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del images, dst, multi, alone
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
