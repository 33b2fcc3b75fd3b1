#!/usr/bin/env python3
"""Dissolves and wipes between plain v210 layers: ONE ph_fused_v210_transition_multi call against the parent's route for the same
frame - one ph_chan_compose_multi call on the equivalent layers - in one process, the sides alternating on warmed shapes, timed with
device events.  The plain 4-layer ph_fused_v210_combine_multi frame of the same size and outputs runs beside them as the floor.  The
layers (with their incoming frames and masks) cycle over a ring of frame sets larger than the 256 MiB Infinity Cache, as bench.py's
headline does.
  python tools/fused_transition_bench.py [reps=1000] [rounds=7] [out=profiles/fused_transition_bench.jsonl] [only=<shape name>]
One JSON line per shape: the median of the rounds for every side and each side's spread (max - min over the rounds).  The new call
counts as faster only if it wins by more than the baseline side's spread.
Kernels alone: run the tool under `rocprofv3 --kernel-trace --stats` with reps=50 rounds=1 and a throw-away out file."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

CACHE_BYTES = 256 << 20
# per shape: its name, the outputs, and per layer None (a cut), ("dissolve", mix), ("wipe", "rgba") or ("wipe", "v210")
SHAPES = [("layer 3 dissolving -> v210", ["v210"], [None, None, None, ("dissolve", 0.375)]),
          ("layer 3 dissolving -> yuv422p8", ["yuv422p8"], [None, None, None, ("dissolve", 0.375)]),
          ("layer 1 dissolving + layer 3 wiping by an f32 mask -> v210+bgra8", ["v210", "bgra8"], [None, ("dissolve", 0.625), None, ("wipe", "rgba")]),
          ("layer 3 wiping by a v210 mask -> v210", ["v210"], [None, None, None, ("wipe", "v210")])]


def main():
    import numpy as np
    import torch
    from phaneron_amd import capi
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "fused_transition_bench.jsonl")
    only = (sys.argv[4] or None) if len(sys.argv) > 4 else None
    ctx = capi.Context(0)
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rspec, wspec, n = "709", "2020", 4
    rd_lut_h, wr_lut_h = capi.gamma2linear_lut(rspec), capi.linear2gamma_lut(wspec)
    rd = (dev(capi.ycbcr2rgb_matrix(rspec)), dev(rd_lut_h), dev(np.concatenate([capi.rgb2rgb_matrix(rspec, wspec), np.zeros(3, np.float32)])))
    wr_lut = dev(wr_lut_h)
    fmts = ("v210", "yuv422p8", "bgra8")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix(wspec, *capi.FORMAT_RANGE[f])) for f in fmts}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], rd_lut_h)
    ctx.register_lut(wr_lut, wr_lut_h)

    def frame(fmt, w, h):
        if fmt == "v210":
            return [torch.empty(capi.v210_pitch_bytes(w) * h, dtype=torch.uint8, device="cuda")]
        return [torch.empty(b, dtype=torch.uint8, device="cuda") for b in capi.pack_plane_bytes(fmt, w, h)]

    lines = []
    for size, w, h in [("2160p", 3840, 2160), ("1080p", 1920, 1080)]:
        frame_bytes = capi.v210_pitch_bytes(w) * h
        ring = CACHE_BYTES // (n * frame_bytes) + 2
        gen = torch.Generator(device="cuda").manual_seed(5)
        words = lambda: torch.randint(0, 2 ** 31 - 1, (frame_bytes // 4,), dtype=torch.int32, device="cuda", generator=gen) & 0x3FFFFFFF
        sets = [[words() for _ in range(n)] for _ in range(ring)]
        incoming = [[words() for _ in range(2)] for _ in range(ring)]  # (at most two layers of a shape are in a transition)
        vmask = [words() for _ in range(ring)]
        fmask = None
        for shape, outs, kinds in SHAPES:
            name = "%s %s" % (size, shape)
            if only and only != name:
                continue
            if fmask is None and any(k and k[1] == "rgba" for k in kinds):
                fmask = [torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=gen) for _ in range(ring)]
            dst = [frame(fmt, w, h) for fmt in outs]
            torch.cuda.synchronize()
            outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
            mine, chan = [], []
            for s in range(ring):
                m, c, taken = [], [], 0
                for i, kind in enumerate(kinds):
                    own = sets[s][i]
                    if kind is None:
                        m.append(own)
                        c.append(dict(src=(own, w, h, None), transition="cut", mix=0.0))
                        continue
                    inc = incoming[s][taken]
                    taken += 1
                    if kind[0] == "dissolve":
                        m.append(dict(v210=own, transition="dissolve", mix=kind[1], incoming=inc))
                        c.append(dict(src=(own, w, h, None), transition="dissolve", mix=kind[1], incoming=(inc, w, h, None)))
                    else:
                        mask = vmask[s] if kind[1] == "v210" else fmask[s]
                        m.append(dict(v210=own, transition="wipe", incoming=inc, mask=mask, mask_format=kind[1]))
                        c.append(dict(src=(own, w, h, None), transition="wipe", mix=0.0, incoming=(inc, w, h, None),
                                      mask=(mask, w, h, None) if kind[1] == "v210" else (mask, w, h, None, "rgba")))
                mine.append(m)
                chan.append(c)
            sides = {"new": [ctx.fused_v210_transition_multi(m, outputs, w, h, *rd, prepare_only=True) for m in mine],
                     "chan_compose_multi": [ctx.chan_compose_multi(c, outputs, w, h, *rd, prepare_only=True) for c in chan],
                     "plain_floor": [ctx.fused_v210_combine_multi(layers, outputs, w, h, *rd, prepare_only=True) for layers in sets]}
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
            base = "chan_compose_multi"
            line = {"bench": "fused_transition", "shape": name, "width": w, "height": h, "layers": n, "frame_sets": ring, "outputs": outs, "reps": reps, "rounds": rounds, "routes": routes,
                    "new_us": round(med["new"], 2), "new_spread_us": round(spread["new"], 2), "baseline": base, "baseline_us": round(med[base], 2),
                    "baseline_spread_us": round(spread[base], 2), "plain_floor_us": round(med["plain_floor"], 2), "plain_floor_spread_us": round(spread["plain_floor"], 2),
                    "saved_us": round(med[base] - med["new"], 2), "new_wins_beyond_spread": bool(med[base] - med["new"] > spread[base]),
                    "rounds_us": {k: [round(x, 2) for x in v] for k, v in us.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del dst, sides, mine, chan
        del sets, incoming, vmask, fmask
    if not only:
        with open(path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
