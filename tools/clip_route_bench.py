#!/usr/bin/env python3
"""A routed channel's file playback: ph_clip_compose_route_multi - the consumers' frames AND the combined f32 RGBA image from the
read-once launches - against the best way there was to make both, timed with device events, in microseconds per frame.  Sides:
  route  the new entry - once with the context option "chan_enlarged" = 1 (one launch of clip_up_route_kernel where the frame is a single
         wire-format clip) and once with 2 (never the one-launch form: the format readers, then compose_up_route)
  chain  ph_pack_read of every clip -> ph_transform of each (-> ph_combine) -> ph_pack_write_multi of the image: the chain the header
         names for a routed channel that plays a file
The sides alternate on warmed shapes inside every round.  The baseline of record is the chain side of a build of the PARENT commit, run in
the same session from a directory of its own: run this file there with mode=baseline (it then never names the new entry) twice in the session -
in front of this build's run and again behind a run of it - and give both files to this build's run of record as parent=<file>,<file>;
their rounds are merged per shape.
The clips are seeded, so every process makes the same frames: a baseline record carries the SHA-256 of the image and the output planes,
and this build compares the new entry's bytes with it - and, byte for byte, with its own chain side - BEFORE it times a shape; a
difference ends the run.
  python tools/clip_route_bench.py [reps=200] [rounds=7] [out=profiles/clip_route_bench.jsonl] [mode=both|baseline] [parent=<jsonl>[,<jsonl>]]
One JSON line per shape and route: every side's median over the rounds, its spread (max - min over the rounds) and its route from a
dry-run trace; whether the entry wins, loses or equals the baseline beyond the larger of the two spreads."""
import ctypes as C
import hashlib
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
    reps = int(pos[0]) if len(pos) > 0 else 200
    rounds = int(pos[1]) if len(pos) > 1 else 7
    path = pos[2] if len(pos) > 2 else os.path.join(ROOT, "profiles", "clip_route_bench.jsonl")
    baseline_only = kw.get("mode", "both") == "baseline"
    parent, parent_sha = {}, {}
    for f in [p for p in kw.get("parent", "").split(",") if p]:
        for line in open(f):
            rec = json.loads(line)
            parent.setdefault(rec["shape"], []).extend(rec["rounds_chain_us"])
            parent_sha.setdefault(rec["shape"], set()).add(rec["sha256"])
    ctx = capi.Context(0)
    lib, hd = capi.lib(), ctx.h
    Q = capi.QUEUE_PROCESS
    stream = ctx.torch_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rd = [dev(capi.ycbcr2rgb_matrix("709")), dev(capi.gamma2linear_lut("709")), dev(np.concatenate([capi.rgb2rgb_matrix("709", "709"), np.zeros(3, np.float32)]))]
    wr_lut = dev(capi.linear2gamma_lut("709"))
    formats = ("v210", "yuv422p10", "yuv420p", "nv12", "rgba8", "p010")
    wr_cm = {f: None if capi.FORMAT_RANGE[f] is None else dev(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE[f])) for f in formats}
    rd_own = {f: dev(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE[f])) if capi.FORMAT_RANGE[f] and capi.FORMAT_RANGE[f][0] == 8 else None for f in formats}
    torch.cuda.synchronize()
    ctx.register_lut(rd[1], capi.gamma2linear_lut("709"))
    ctx.register_lut(wr_lut, capi.linear2gamma_lut("709"))
    R = 4  # a ring of frames: no clip is read from the cache the launch before left it in
    gen = torch.Generator(device="cuda")

    def planes(fmt, w, h, random=False):
        sizes = [capi.v210_pitch_bytes(w) * h] if fmt == "v210" else capi.pack_plane_bytes(fmt, w, h)
        if random:  # (codes of any value: only the time counts)
            return [torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen) for n in sizes]
        return [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in sizes]

    HD, UHD, P720 = (1920, 1080), (3840, 2160), (1280, 720)
    fill, inset = dict(), dict(scale_x=0.8, scale_y=0.8, offset_x=0.1, offset_y=-0.1)
    # (name, [(clip format, clip size, placement)], channel size, outputs)
    shapes = [("1080p yuv420p on 1080p -> image + v210", [("yuv420p", HD, fill)], HD, ["v210"]),
              ("1080p yuv420p on 1080p -> image + v210 + rgba8", [("yuv420p", HD, fill)], HD, ["v210", "rgba8"]),
              ("1080p yuv420p on 1080p -> the image alone", [("yuv420p", HD, fill)], HD, []),
              ("720p yuv420p filling 1080p -> image + nv12", [("yuv420p", P720, fill)], HD, ["nv12"]),
              ("1080p p010 on 2160p -> image + yuv422p10", [("p010", HD, fill)], UHD, ["yuv422p10"]),
              ("two 720p yuv422p10 clips on 1080p -> image + v210", [("yuv422p10", P720, fill), ("yuv422p10", P720, inset)], HD, ["v210"])]
    lines = []
    for index, (name, clips, (w, h), outs) in enumerate(shapes):
        gen.manual_seed(20261021 + index)
        ring, keep = [], []
        for _ in range(R):
            layers = []
            for fmt, (sw, sh), place in clips:
                p = planes(fmt, sw, sh, random=True)
                layers.append(dict(src=(tuple(p), sw, sh, capi.transform_matrix(w, h, **place), fmt, rd_own[fmt]), transition="cut", mix=0.0))
            ring.append(layers)
        dst = [planes(fmt, w, h) for fmt in outs]
        image = torch.full((w * h * 16,), 0x5A, dtype=torch.uint8, device="cuda")
        # the chain's own images: every clip's read image and placed image, as a channel's operators allocate them
        small = [torch.empty(sw * sh * 16, dtype=torch.uint8, device="cuda") for _, (sw, sh), _ in clips]
        placed = [torch.empty(w * h * 16, dtype=torch.uint8, device="cuda") for _ in clips] if len(clips) > 1 else [image]
        mats = [dev(capi.transform_matrix(w, h, **place)) for _, _, place in clips]
        torch.cuda.synchronize()
        outputs = [dict(fmt=fmt, planes=d, interlace=0, wr_cm=wr_cm[fmt], wr_lut=wr_lut) for fmt, d in zip(outs, dst)]
        c_outs = ctx._chan_outputs(outputs)
        chain_calls = []
        for s in range(R):
            calls = []
            for i, (fmt, (sw, sh), _) in enumerate(clips):
                arr = (C.c_void_p * 3)(*([p.data_ptr() for p in ring[s][i]["src"][0]] + [None] * (3 - len(ring[s][i]["src"][0]))))
                keep.append(arr)
                calls.append((lib.ph_pack_read, (hd, Q, capi.FORMATS[fmt], arr, ptr(small[i]), sw, sh, ptr(rd_own[fmt] if rd_own[fmt] is not None else rd[0]), ptr(rd[1]), ptr(rd[2]))))
                calls.append((lib.ph_transform, (hd, Q, ptr(small[i]), sw, sh, ptr(mats[i]), ptr(placed[i]), w, h)))
            if len(clips) > 1:
                arr = (C.c_void_p * len(clips))(*[p.data_ptr() for p in placed])
                keep.append(arr)
                calls.append((lib.ph_combine, (hd, Q, len(clips), arr, w, h, ptr(image))))
            if outs:
                calls.append((lib.ph_pack_write_multi, (hd, Q, ptr(image), len(outs), c_outs, w, h)))
            chain_calls.append(calls)

        def chain(i):
            for fn, args in chain_calls[i]:
                capi.check(fn(*args), hd)
        route = None if baseline_only else [ctx.clip_compose_route_multi(ring[s], image, outputs, w, h, *rd, prepare_only=True) for s in range(R)]

        def frame_of(fn):
            """the image and the output planes of frame 0 of the ring, as bytes"""
            for p in [image] + [p for d in dst for p in d]:
                p.fill_(0x5A)
            torch.cuda.synchronize()
            fn(0)
            ctx.wait()
            torch.cuda.synchronize()
            return [image.cpu().numpy().tobytes()] + [p.cpu().numpy().tobytes() for d in dst for p in d]

        def sha(frame):
            hsh = hashlib.sha256()
            for b in frame:
                hsh.update(b)
            return hsh.hexdigest()

        for option in ([1] if baseline_only else [1, 2]):
            shape = name if baseline_only else "%s [chan_enlarged=%d]" % (name, option)
            sides = {"chain": chain}
            if not baseline_only:
                sides["route"] = lambda i: route[i]()
            # the bytes first: nothing is timed that does not make the baseline's image and frames
            ctx.set_option("chan_enlarged", option)
            frames = {k: frame_of(fn) for k, fn in sides.items()}
            digest = sha(frames["chain"])
            if not baseline_only:
                assert frames["route"] == frames["chain"], "%s: the entry's image or planes differ from the chain's" % shape
                assert not parent_sha.get(name) or parent_sha[name] == {digest}, "%s: the bytes differ from the parent build's (%s against %s)" % (shape, digest, parent_sha[name])
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
                return 1e3 * e0.elapsed_time(e1) / reps
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
            ctx.set_option("chan_enlarged", 1)
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = {k: max(v) - min(v) for k, v in us.items()}
            line = {"bench": "clip_route", "shape": shape if not baseline_only else name, "clips": [[fmt, sw, sh] for fmt, (sw, sh), _ in clips], "width": w, "height": h,
                    "outputs": outs, "reps": reps, "rounds": rounds, "unit": "us per frame", "routes": routes, "sha256": digest, "chain_us": round(med["chain"], 2),
                    "chain_spread_us": round(spread["chain"], 2), "rounds_chain_us": [round(v, 2) for v in us["chain"]]}
            if not baseline_only:
                line.update({"chan_enlarged": option, "route_us": round(med["route"], 2), "route_spread_us": round(spread["route"], 2), "rounds_route_us": [round(v, 2) for v in us["route"]]})
                base, base_spread, which = med["chain"], spread["chain"], "chain (this build)"
                if name in parent:
                    base, base_spread, which = statistics.median(parent[name]), max(parent[name]) - min(parent[name]), "chain (parent build, same session)"
                    line.update({"parent_chain_us": round(base, 2), "parent_chain_spread_us": round(base_spread, 2), "rounds_parent_chain_us": parent[name],
                                 "bytes_equal_parent": True})
                worst = max(spread["route"], base_spread)
                saved = base - med["route"]
                line.update({"baseline": which, "saved_us": round(saved, 2), "verdict": "wins" if saved > worst else "loses" if -saved > worst else "equal within spread"})
            print(json.dumps(line), flush=True)
            lines.append(line)
        del ring, dst, route, chain_calls, keep
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
