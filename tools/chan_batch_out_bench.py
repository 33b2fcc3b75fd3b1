#!/usr/bin/env python3
"""Several channels' frames for consumers other than SDI: ONE ph_chan_compose_batch_out call against the way the same frames are made
without it - one ph_chan_compose (one output) or ph_chan_compose_multi (several) call per channel - in one process, the two sides
alternating on warmed shapes, timed with device events.  Every channel runs BASELINE config 2's program (four v210 layers: a
background, three insets, a wipe in progress) on sources of its own.  The last shape guards the v210 frames: four channels for SDI alone
against ph_chan_compose_batch, which has the same phase 1.
  python tools/chan_batch_out_bench.py [reps=200] [rounds=7] [out=profiles/chan_batch_out_bench.jsonl] [only=<shape name>: for a profiler run]
One JSON line per shape: both sides' medians over the rounds per call and per channel frame, both sides' run-to-run spread (max - min
over the rounds), and whether the shared launch wins by more than the separate side's spread."""
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
    rounds = max(7, int(sys.argv[2])) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "chan_batch_out_bench.jsonl")
    only = sys.argv[4] if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    cm8 = dev(capi.rgb2ycbcr_matrix("709", 8, 16, 235, 224))
    wr_cm = {"v210": dev(capi.rgb2ycbcr_matrix("709")), "yuv422p8": cm8, "nv12": cm8, "rgba8": None, "bgra8": None}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of source sets per channel: no frame is read from the cache the launch before left it in

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda")]
        if fmt == "yuv422p8":
            return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in (w * h, w * h // 2, w * h // 2)]
        if fmt == "nv12":
            return [torch.empty(n, dtype=torch.uint8, device="cuda") for n in (w * h, w * h // 2)]
        return [torch.empty(w * h, dtype=torch.int32, device="cuda")]

    def config2(w, h, channels):
        """[ring slot][channel] -> the channel's layers"""
        words = capi.v210_pitch_bytes(w) * h // 4
        mask = torch.zeros(h, w, 4, device="cuda")
        mask[..., 0] = torch.linspace(0, 1, w, device="cuda")[None, :]
        mask = mask.reshape(-1).contiguous()
        mats = [capi.transform_matrix(w, h)] + [capi.transform_matrix(w, h, scale_x=0.5, scale_y=0.5, offset_x=ox, offset_y=oy) for ox, oy in ((-0.25, -0.25), (0.25, -0.25), (0.25, 0.25))]
        ring = []
        for _ in range(R):
            chans = []
            for _ in range(channels):
                s = [torch.randint(0, 2 ** 30, (words,), dtype=torch.int32, device="cuda") for _ in range(5)]
                ls = [dict(src=(s[l], w, h, mats[l])) for l in range(4)]
                ls[3].update(transition="wipe", incoming=(s[4], w, h, None), mask=(mask, w, h, None, "rgba"))
                chans.append(ls)
            ring.append(chans)
        return ring

    shapes = [("4 x config2 1080p -> yuv422p8", 1920, 1080, 4, [("yuv422p8", 0)]),
              ("4 x config2 1080p -> v210+bgra8", 1920, 1080, 4, [("v210", 0), ("bgra8", 0)]),
              ("4 x config2 720p -> nv12", 1280, 720, 4, [("nv12", 0)]),
              ("2 x config2 1080p -> v210+yuv422p8+rgba8", 1920, 1080, 2, [("v210", 0), ("yuv422p8", 0), ("rgba8", 0)]),
              ("4 x config2 1080p -> v210 (against ph_chan_compose_batch)", 1920, 1080, 4, [("v210", 0)])]
    lines = []
    for name, w, h, channels, outs in shapes:
        if only and only != name:
            continue
        ring = config2(w, h, channels)
        dst = [[frame(fmt, w, h) for fmt, _ in outs] for _ in range(channels)]
        torch.cuda.synchronize()
        outputs = [[dict(fmt=fmt, planes=d, interlace=il, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for (fmt, il), d in zip(outs, dst[c])] for c in range(channels)]
        together = [ctx.chan_compose_batch_out([(chans[c], outputs[c]) for c in range(channels)], w, h, *rd, prepare_only=True) for chans in ring]
        # the parent's way of making the same frames
        if outs == [("v210", 0)]:
            separate = [[ctx.chan_compose_batch([(chans[c], dst[c][0][0], 0) for c in range(channels)], w, h, *rd, wr_cm["v210"], wr_lut, prepare_only=True)] for chans in ring]
            baseline = "ph_chan_compose_batch, one call"
        elif len(outs) == 1:
            fmt, il = outs[0]
            separate = [[ctx.chan_compose_v210(chans[c], dst[c][0], w, h, il, *rd, wr_cm[fmt], wr_lut, prepare_only=True, out_fmt=fmt) for c in range(channels)] for chans in ring]
            baseline = "ph_chan_compose per channel"
        else:
            separate = [[ctx.chan_compose_multi(chans[c], outputs[c], w, h, *rd, prepare_only=True) for c in range(channels)] for chans in ring]
            baseline = "ph_chan_compose_multi per channel"
        routes = {}
        with capi.trace(dry_run=True) as t:
            together[0]()
        routes["batch_out"] = t.route
        with capi.trace(dry_run=True) as t:
            for job in separate[0]:
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
        sides = {"batch_out": lambda i: together[i](), "separate": lambda i: [job() for job in separate[i]]}
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
        spread = {k: max(v) - min(v) for k, v in us.items()}
        line = {"bench": "chan_batch_out", "shape": name, "width": w, "height": h, "channels": channels, "outputs": ["%s il %d" % o for o in outs], "baseline": baseline,
                "reps": reps, "rounds": rounds, "routes": routes,
                "batch_out_us": round(med["batch_out"], 2), "separate_us": round(med["separate"], 2),
                "batch_out_us_per_channel_frame": round(med["batch_out"] / channels, 2), "separate_us_per_channel_frame": round(med["separate"] / channels, 2),
                "batch_out_spread_us": round(spread["batch_out"], 2), "separate_spread_us": round(spread["separate"], 2),
                "saved_us": round(med["separate"] - med["batch_out"], 2),
                "batch_out_wins_beyond_spread": bool(med["separate"] - med["batch_out"] > spread["separate"]),
                "batch_out_loses_beyond_spread": bool(med["batch_out"] - med["separate"] > spread["separate"]),
                "rounds_batch_out_us": [round(v, 2) for v in us["batch_out"]], "rounds_separate_us": [round(v, 2) for v in us["separate"]]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del ring, dst, outputs, together, separate
        torch.cuda.empty_cache()
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
