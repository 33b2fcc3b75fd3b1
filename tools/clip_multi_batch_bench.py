#!/usr/bin/env python3
"""Several channels' file playback per tick: ph_clip_compose_batch_out against the same frames as n consecutive ph_clip_compose_multi
calls, timed with device events, in microseconds per channel frame.  Sides:
  batch  the new entry, one call for the n channels (one launch of clip_up_multi_kernel<.., MULTI> where the jobs share)
  multi  n consecutive ph_clip_compose_multi calls on the same arguments, this build: what a tick costs without the entry
The sides alternate on warmed shapes inside every round.  The baseline of record is the multi side of a build of the PARENT commit, run in
the same session: run this file from a checkout of the parent with mode=baseline (it then never names the new entry) in front of and
behind the run of this build, and give both files to this build's run as parent=<file>,<file>; their rounds are merged per shape.
Shapes: four 1080p yuv420p channels -> nv12; four 720p yuv420p clips on 1080p channels -> v210 + rgba8; two and three 1080p p010 channels
-> yuv422p10 + rgba8; four 1080p yuv420p channels -> v210 alone (the entry hands every job to ph_chan_compose: must equal the baseline).
  python tools/clip_multi_batch_bench.py [reps=100] [rounds=7] [out=profiles/clip_multi_batch_bench.jsonl] [mode=both|baseline] [parent=<jsonl>[,<jsonl>]]
One JSON line per shape: every side's median over the rounds, its spread (max - min over the rounds) and its route from a dry-run trace;
whether the entry wins, loses or equals the baseline beyond the larger of the two spreads."""
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
    pos = [a for a in sys.argv[1:] if "=" not in a]
    kw = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    reps = int(pos[0]) if len(pos) > 0 else 100
    rounds = int(pos[1]) if len(pos) > 1 else 7
    path = pos[2] if len(pos) > 2 else os.path.join(ROOT, "profiles", "clip_multi_batch_bench.jsonl")
    baseline_only = kw.get("mode", "both") == "baseline"
    parent = {}
    for f in [p for p in kw.get("parent", "").split(",") if p]:
        for line in open(f):
            rec = json.loads(line)
            parent.setdefault(rec["shape"], []).extend(rec["rounds_multi_us"])
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    formats = ("v210", "yuv422p10", "yuv420p", "nv12", "rgba8", "p010")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE[f])) for f in formats}
    rd_own = {f: dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE[f])) if capi.FORMAT_RANGE[f] and capi.FORMAT_RANGE[f][0] == 8 else None for f in formats}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 3  # a ring of ticks: no clip is read from the cache the tick before left it in

    def planes(fmt, w, h, random=False):
        sizes = [capi.v210_pitch_bytes(w) * h] if fmt == "v210" else capi.pack_plane_bytes(fmt, w, h)
        if random:  # (8-bit codes of any value: only the time counts)
            return [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda") for n in sizes]
        return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in sizes]

    HD, P720 = (1920, 1080), (1280, 720)
    # (name, channels, clip format, clip size, channel size, outputs)
    shapes = [("4 x 1080p yuv420p fill -> nv12", 4, "yuv420p", HD, HD, ["nv12"]),
              ("4 x 720p yuv420p on 1080p -> v210+rgba8", 4, "yuv420p", P720, HD, ["v210", "rgba8"]),
              ("2 x 1080p p010 fill -> yuv422p10+rgba8", 2, "p010", HD, HD, ["yuv422p10", "rgba8"]),
              ("3 x 1080p p010 fill -> yuv422p10+rgba8", 3, "p010", HD, HD, ["yuv422p10", "rgba8"]),
              ("4 x 1080p yuv420p fill -> v210 alone", 4, "yuv420p", HD, HD, ["v210"])]
    lines = []
    for name, n, fmt, (sw, sh), (w, h), outs in shapes:
        ticks = []  # per tick of the ring: the n channels' (layers, outputs)
        for _ in range(R):
            jobs = []
            for _ in range(n):
                layers = [dict(src=(tuple(planes(fmt, sw, sh, random=True)), sw, sh, capi.transform_matrix(w, h), fmt, rd_own[fmt]))]
                jobs.append((layers, [dict(fmt=f, planes=planes(f, w, h), interlace=0, wr_cm=wr_cm[f], wr_lut=wr_lut) for f in outs]))
            ticks.append(jobs)
        torch.cuda.synchronize()
        multi = [[ctx.clip_compose_multi(layers, outputs, w, h, *rd, prepare_only=True) for layers, outputs in jobs] for jobs in ticks]
        sides = {"multi": lambda i: [call() for call in multi[i]]}
        if not baseline_only:
            batch = [ctx.clip_compose_batch_out(jobs, w, h, *rd, prepare_only=True) for jobs in ticks]
            sides["batch"] = lambda i: batch[i]()
        routes = {}
        for k, fn in sides.items():
            with capi.trace(dry_run=True) as t:
                fn(0)
            routes[k] = t.route

        def timed(k):
            fn = sides[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for i in range(reps):
                fn(i % R)
            e1.record(stream)
            ctx.wait()
            return 1e3 * e0.elapsed_time(e1) / (reps * n)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # until every shape is warm and the clocks have settled
            for k in sides:
                for i in range(R):
                    sides[k](i)
            ctx.wait()
        us = {k: [] for k in sides}
        for _ in range(rounds):  # the sides alternate inside a round
            for k in sides:
                us[k].append(timed(k))
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        line = {"bench": "clip_multi_batch", "shape": name, "channels": n, "clip": [fmt, sw, sh], "width": w, "height": h, "outputs": outs, "reps": reps, "rounds": rounds,
                "unit": "us per channel frame", "routes": routes, "multi_us": round(med["multi"], 2), "multi_spread_us": round(spread["multi"], 2),
                "rounds_multi_us": [round(v, 2) for v in us["multi"]]}
        if not baseline_only:
            line.update({"batch_us": round(med["batch"], 2), "batch_spread_us": round(spread["batch"], 2), "rounds_batch_us": [round(v, 2) for v in us["batch"]]})
            base, base_spread, which = med["multi"], spread["multi"], "multi (this build)"
            if name in parent:
                base, base_spread, which = statistics.median(parent[name]), max(parent[name]) - min(parent[name]), "multi (parent build, same session)"
                line.update({"parent_multi_us": round(base, 2), "parent_multi_spread_us": round(base_spread, 2), "rounds_parent_multi_us": parent[name]})
            worst = max(spread["batch"], base_spread)
            saved = base - med["batch"]
            line.update({"baseline": which, "saved_us": round(saved, 2), "verdict": "wins" if saved > worst else "loses" if -saved > worst else "equal within spread"})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del ticks, multi
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
