#!/usr/bin/env python3
"""File playback for consumers other than one v210 frame: ph_clip_compose_multi against what the same frames cost without it, in one
process, the sides alternating on warmed shapes, timed with device events.  Sides:
  clip  the new entry (one launch of clip_up_multi_kernel per writer table for a single clip; two stages for several)
  chan  ph_chan_compose_multi on the same arguments - what these frames took before the entry existed: the baseline
  two   the new entry with the context option "chan_enlarged" = 2 (never the one-launch form: the format's reader, then compose_up_multi)
Shapes: a 1080p yuv420p clip under the default fill on a 1080p channel to yuv420p, nv12, rgba8, v210 + rgba8, v210 + yuv422p8 + rgba8; a
720p yuv420p clip filling a 1080p channel to nv12 and to v210 + rgba8; a 1080p p010 clip on a 2160p channel to yuv422p10; two 720p yuv422p10
clips on a 1080p channel to yuv422p8 (n = 2: the entry takes two stages; recorded so that a later change can decide).
  python tools/clip_multi_bench.py [reps=200] [rounds=7] [out=profiles/clip_multi_bench.jsonl] [only=<shape name>]
One JSON line per shape: the median of the rounds for every side, every side's spread (max - min over the rounds) and its route from a
dry-run trace."""
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
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "clip_multi_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    formats = ("v210", "yuv422p10", "yuv422p8", "yuv420p", "nv12", "rgba8", "p010")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE[f])) for f in formats}
    rd_own = {f: dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE[f])) if capi.FORMAT_RANGE[f] and capi.FORMAT_RANGE[f][0] == 8 else None for f in formats}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of clips: no clip is read from the cache the launch before left it in

    def planes(fmt, w, h, random=False):
        sizes = [capi.v210_pitch_bytes(w) * h] if fmt == "v210" else capi.pack_plane_bytes(fmt, w, h)
        if random:  # (8-bit codes of any value: only the time counts)
            return [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda") for n in sizes]
        return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in sizes]

    HD, UHD, P720 = (1920, 1080), (3840, 2160), (1280, 720)
    # (name, [(clip format, clip size, placement)], channel size, outputs)
    shapes = [("1080p yuv420p fill -> yuv420p", [("yuv420p", HD, {})], HD, ["yuv420p"]),
              ("1080p yuv420p fill -> nv12", [("yuv420p", HD, {})], HD, ["nv12"]),
              ("1080p yuv420p fill -> rgba8", [("yuv420p", HD, {})], HD, ["rgba8"]),
              ("1080p yuv420p fill -> v210+rgba8", [("yuv420p", HD, {})], HD, ["v210", "rgba8"]),
              ("1080p yuv420p fill -> v210+yuv422p8+rgba8", [("yuv420p", HD, {})], HD, ["v210", "yuv422p8", "rgba8"]),
              ("720p yuv420p on 1080p -> nv12", [("yuv420p", P720, {})], HD, ["nv12"]),
              ("720p yuv420p on 1080p -> v210+rgba8", [("yuv420p", P720, {})], HD, ["v210", "rgba8"]),
              ("1080p p010 on 2160p -> yuv422p10", [("p010", HD, {})], UHD, ["yuv422p10"]),
              ("two 720p yuv422p10 on 1080p -> yuv422p8", [("yuv422p10", P720, {}), ("yuv422p10", P720, dict(scale_x=0.8, scale_y=0.8))], HD, ["yuv422p8"])]
    lines = []
    for name, clips, (w, h), outs in shapes:
        if only and only != name:
            continue
        ring = [[(tuple(planes(fmt, sw, sh, random=True)), sw, sh, capi.transform_matrix(w, h, **kw), fmt, rd_own[fmt]) for fmt, (sw, sh), kw in clips] for _ in range(R)]
        for s in range(R):
            ring[s] = [dict(src=(c[0][0], c[1], c[2], c[3]) if c[4] == "v210" else c) for c in ring[s]]
        dst = [planes(fmt, w, h) for fmt in outs]
        torch.cuda.synchronize()
        outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
        clip = [ctx.clip_compose_multi(ring[s], outputs, w, h, *rd, prepare_only=True) for s in range(R)]
        chan = [ctx.chan_compose_multi(ring[s], outputs, w, h, *rd, prepare_only=True) for s in range(R)]
        option = {"clip": 1, "chan": 1, "two": 2}
        sides = {"clip": lambda i: clip[i](), "chan": lambda i: chan[i](), "two": lambda i: clip[i]()}
        routes = {}
        for k, fn in sides.items():
            ctx.set_option("chan_enlarged", option[k])
            with capi.trace(dry_run=True) as t:
                fn(0)
            routes[k] = t.route
        ctx.set_option("chan_enlarged", 1)

        def timed(k):
            ctx.set_option("chan_enlarged", option[k])  # (read when a call chooses its route; set once per timed run, outside the events)
            fn = sides[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                fn(i % R)
            e1.record(stream)
            ctx.wait()
            ctx.set_option("chan_enlarged", 1)
            return 1e3 * e0.elapsed_time(e1) / reps
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # until every shape is warm and the clocks have settled
            for k in sides:
                ctx.set_option("chan_enlarged", option[k])
                for i in range(R):
                    sides[k](i)
            ctx.wait()
        ctx.set_option("chan_enlarged", 1)
        us = {k: [] for k in sides}
        for _ in range(rounds):  # the sides alternate inside a round
            for k in sides:
                us[k].append(timed(k))
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        worst = max(spread["clip"], spread["chan"])
        line = {"bench": "clip_multi", "shape": name, "clips": [[fmt, sw, sh] for fmt, (sw, sh), _ in clips], "width": w, "height": h, "outputs": outs, "reps": reps, "rounds": rounds,
                "routes": routes, "clip_us": round(med["clip"], 2), "chan_us": round(med["chan"], 2), "two_us": round(med["two"], 2),
                "clip_spread_us": round(spread["clip"], 2), "chan_spread_us": round(spread["chan"], 2), "two_spread_us": round(spread["two"], 2),
                "saved_us": round(med["chan"] - med["clip"], 2), "clip_wins_beyond_spread": bool(med["chan"] - med["clip"] > worst),
                "equal_within_spread": bool(abs(med["chan"] - med["clip"]) <= worst),
                "rounds_clip_us": [round(v, 2) for v in us["clip"]], "rounds_chan_us": [round(v, 2) for v in us["chan"]], "rounds_two_us": [round(v, 2) for v in us["two"]]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del ring, dst, clip, chan
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
